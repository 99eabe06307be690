// train_deepset.hip -- the per-trial part of the amortizer's DeepSet summary network (bayesflow_nddms_amd/amortizer.py::
// InvariantNetwork; the stand-in for bf.networks.InvariantNetwork, basic_ddm_dc.py:163) for the online-training loop
// (basic_ddm_dc.py:199-202): every 3-layer MLP that runs on each trial of each set -- Linear, ReLU, Linear, ReLU, Linear, hidden
// width 64 -- as ONE kernel forward and ONE backward, with what surrounds it fused in:
//   * a per-set context vector (the masked mean over the set's trials of another MLP's output, taken through the context columns
//     of W1) added before the first ReLU: the "equivariant" half of a DeepSet block;
//   * the masked per-set sums of the output: the "invariant" half and the final pooling;
//   * backward: the weight gradients as per-workgroup partial sums (deterministic; one reduction kernel sums them), the input
//     gradient, the context's gradient, the pooled output's gradient spread back over the set's trials.
// In PyTorch each Linear / ReLU / mask / sum / concat / expand is a launch of 4-7 microseconds over [32 sets x <= 300 trials, 64]:
// ~150 launches per training iteration.  Here the [rows, 64] x [64, 64] products are v_mfma_f32_32x32x2_f32 (exact f32: a k-ordered
// fmaf chain) on LDS tiles of 64 rows; a workgroup owns up to `rows_per_wg` consecutive trials of ONE set, so pooling and context
// never cross a workgroup inside a kernel -- they cross KERNELS as [set, workgroup-of-the-set, 64] partial sums.
// Every step of a layer is written ONCE ("the forward steps", "the backward steps"); the four kernels are sequences of those calls, so the
// kernels that run two MLPs in one launch write what two launches of the single kernels write, bit for bit
// (tests/test_gpu_deepset_pairs.py).
// Inference (nddm_deepset_summary, at the end of the forward section): the same forward steps with nothing saved for a backward and a
// trial count PER SET -- the whole summary network of a batch of data sets of different sizes in blocks + 2 launches
// (tests/test_gpu_ragged_summary.py).
// gfx950 only.  tests/test_gpu_training.py compares with the PyTorch composition.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nddm_deepset {

constexpr int HS = 64;        // hidden width
constexpr int LD = HS + 4;    // LDS row stride: 16-byte aligned rows, and the operand reads of one wave instruction touch every bank twice
constexpr int TM = 64;        // rows per tile
constexpr int NT = 256;       // threads per workgroup: wave w owns the 32 x 32 tile (w >> 1, w & 1) of every 64 x 64 product
constexpr int DS_MAX = 4;     // a "small" input (the raw trials: rt, choice) goes through layer 1 as plain FMAs
constexpr int NQ = HS * HS / 4 / NT;      // 16-byte pieces per thread of a [64][64] tile (of weights, or of TM == HS rows)
static_assert(TM == HS, "a row tile and a weight matrix are staged by the same pair of functions");
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));      // (register arrays of HIP's float4 STRUCT were seen kept in memory; of this type not)

#ifdef NDDM_TRAIN_STAMPS      // development only: phase time stamps of one workgroup (tools/train_stamps.py)
__device__ unsigned long long g_stamps[8192];
__device__ int g_nstamps;
#ifndef NDDM_STAMP_BLOCK
#define NDDM_STAMP_BLOCK 0
#endif
#define STAMP(id) do { if (threadIdx.x == 0 && blockIdx.x == NDDM_STAMP_BLOCK) { int k_ = g_nstamps++; if (k_ < 4096) { g_stamps[2 * k_] = (id); g_stamps[2 * k_ + 1] = wall_clock64(); } } } while (0)
#else
#define STAMP(id) do { } while (0)
#endif

struct Mlp { const float *W1; int ldw1; const float *b1, *W2, *b2, *W3, *b3; };
// W1 [64, ldw1]: columns [0, d_in) act on the trial, columns [d_in, d_in + 64) on the set's pooled context (if there is one)

struct Common {
    const float *x; int d_in;               // [B * N, d_in]
    int B, N, S, rows_per_wg;               // S workgroups per set
    const float *mask; int mask_is_count;   // [N]: 1 = a real trial, 0 = padding; null: all real.  mask_is_count: ONE float, the number
                                            // of real trials n (device scalar): trial i is real iff i < n, and 1 / n is taken from it
    const float *inv_n; float inv_n_host;   // 1 / (number of real trials): device scalar, or (null) the host's value
    const float *ctx_part; int S_ctx;       // [B, S_ctx, 64] partial sums of the pooled producer; null: no context
    Mlp P;
    int d_out;                              // rows of W3 / b3 (<= 64): 64 for the per-trial MLPs, the summary width for the last MLP
    const float *x_part; int S_x;           // not null (d_in == 64): row r of x IS inv_n * sum over s of x_part[r][s][.] -- the MLP
};                                          // after the pooling runs on the pooled means, one row per set (launched as ONE "set" of B rows)

// What a thread is in the workgroup.  Of a 64 x 64 product: wave w owns the 32 x 32 tile (rb, ub), the lane holds row / column m of
// the operands for the 32 k's of half kk, and column u of every result tile.  Of a per-column pass: unit uu, rows 16 rg ...
struct Lane {
    int t, lane, wave, m, kk, rb, ub, u, uu, rg;
    __device__ __forceinline__ Lane()
        : t(threadIdx.x), lane(t & 63), wave(t >> 6), m(lane & 31), kk(lane >> 5), rb(wave >> 1), ub(wave & 1), u(32 * ub + m), uu(t & 63), rg(t >> 6) {}
};
// What the workgroup owns: trials [n_begin, n_end) of set b, as the set's workgroup sp (wg: its row of every [B, S, .] array)
struct Span {
    int b, sp, n_begin, n_end, wg;
    long long row0;                         // the set's first row of every [B * N, .] array
    __device__ __forceinline__ Span(const Common &C) : Span(C, C.N) {}
    // ... of a set whose rows end at n_valid <= N (inference: the set's own count; n_end <= n_begin: the workgroup owns no trial)
    __device__ __forceinline__ Span(const Common &C, int n_valid)
        : b(blockIdx.x / C.S), sp(blockIdx.x - b * C.S), n_begin(sp * C.rows_per_wg), n_end(min(n_valid, n_begin + C.rows_per_wg)), wg(blockIdx.x),
          row0((long long)b * C.N) {}
};
// Inference (nddm_deepset_summary): every set has its own number of real trials, its first n[b] of n_max (null: n_max of every set)
struct SetCounts {
    const int *n; int n_max;
    __device__ __forceinline__ int of(int b) const { return n ? min(max(n[b], 0), n_max) : n_max; }
    __device__ __forceinline__ float inv(int b) const { return 1.0f / (float)of(b); }
};

// acc += A B over 64 k's.  Lane l holds A[i = l & 31][k] and B[k][j = l & 31] for the 32 k's of its half (l >> 5): the order of
// the sum is free, so step s of the instruction stream takes k = 32 (l >> 5) + s from both.  SA / SB: distance in floats between
// consecutive k's of this lane's operand (1: along a row of the LDS tile -- 16-byte reads; LD: down a column).
template <int SA, int SB>
__device__ __forceinline__ f32x16 mma64(const float *ap, const float *bp, f32x16 acc)
{
    float a[32], b[32];
    if (SA == 1) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float4 v = *reinterpret_cast<const float4 *>(ap + 4 * q);
            a[4 * q] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int s = 0; s < 32; ++s) a[s] = ap[s * SA];
    }
    if (SB == 1) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float4 v = *reinterpret_cast<const float4 *>(bp + 4 * q);
            b[4 * q] = v.x; b[4 * q + 1] = v.y; b[4 * q + 2] = v.z; b[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int s = 0; s < 32; ++s) b[s] = bp[s * SB];
    }
#pragma unroll
    for (int s = 0; s < 32; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
    return acc;
}
// register v of lane l of a result tile: row (v & 3) + 8 (v >> 2) + 4 (l >> 5), column l & 31
__device__ __forceinline__ int drow(int v, int kk) { return (v & 3) + 8 * (v >> 2) + 4 * kk; }

__device__ __forceinline__ f32x16 zero16()
{
    f32x16 z;
#pragma unroll
    for (int q = 0; q < 16; ++q) z[q] = 0.0f;
    return z;
}

// [rows <= 64] x 64 of a row-major array (ldw: its row stride in floats, a multiple of 4) -> LDS [64][LD] (rows beyond: zero),
// 16-byte loads, in two halves: the loads into registers now (from a clamped row: no branch), the stores to LDS when the buffer's
// last readers are done / its first reader is about to run -- a kernel that issues EVERY load up front and stores each operand just
// before the phase that needs it exposes one load latency instead of one per operand
__device__ __forceinline__ void fetch64(f32x4 (&v)[NQ], const float *src, int ldw, int t, int rows = HS)
{
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const int p = t + NT * k, r = p >> 4, c4 = p & 15;
        v[k] = *reinterpret_cast<const f32x4 *>(src + (long long)min(r, rows - 1) * ldw + 4 * c4);
    }
}
__device__ __forceinline__ void store64(float (*dst)[LD], const f32x4 (&v)[NQ], int t, int rows = HS)
{
    const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const int p = t + NT * k, r = p >> 4, c4 = p & 15;
        *reinterpret_cast<f32x4 *>(&dst[r][4 * c4]) = r < rows ? v[k] : z;
    }
}
// the same pair for the tile of rows n0 .. n0 + 63 of the workgroup's set in a [B * N, 64] array (saved activations, an input, a
// gradient): rows beyond the workgroup's range are fetched from its last row and zeroed at the store
__device__ __forceinline__ void fetch_tile(f32x4 (&v)[NQ], const float *src, const Span &W, int n0, int t)
{
    fetch64(v, src + (W.row0 + n0) * HS, HS, t, W.n_end - n0);
}
__device__ __forceinline__ void store_tile(float (*dst)[LD], const f32x4 (&v)[NQ], const Span &W, int n0, int t)
{
    store64(dst, v, t, W.n_end - n0);
}

// sum over s = 0 .. S - 1 of p[s * stride], added in that order -- with the loads of eight terms in flight at a time: as a plain loop
// (the trip count is a kernel argument) every term waited for its own round trip to L2, 5 x ~0.6 us at the head of a kernel
__device__ __forceinline__ float sum_in_order(const float *p, int S, long long stride)
{
    float a = 0.0f;
    for (int s0 = 0; s0 < S; s0 += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[(long long)min(s0 + k, S - 1) * stride];
#pragma unroll
        for (int k = 0; k < 8; ++k) a += s0 + k < S ? v[k] : 0.0f;
    }
    return a;
}

// four columns of row `row` of the input of a 64-wide MLP: loaded, or (x_part) the mean of the pooled partial sums
__device__ __forceinline__ float4 x_row4(const Common &C, long long row, int c4, float inv_n)
{
    if (!C.x_part) return *reinterpret_cast<const float4 *>(C.x + row * HS + 4 * c4);
    float4 a = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int s0 = 0; s0 < C.S_x; s0 += 8) {          // (eight partial rows in flight, added in order: see sum_in_order)
        float4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = *reinterpret_cast<const float4 *>(C.x_part + (row * C.S_x + min(s0 + k, C.S_x - 1)) * HS + 4 * c4);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float f = s0 + k < C.S_x ? 1.0f : 0.0f;
            a.x += f * v[k].x; a.y += f * v[k].y; a.z += f * v[k].z; a.w += f * v[k].w;
        }
    }
    a.x *= inv_n; a.y *= inv_n; a.z *= inv_n; a.w *= inv_n;
    return a;
}
// fetch_tile of a 64-wide input (store_tile stores it).  rows: not null (the MLP after the pooling at inference, one row per set):
// every row takes the 1 / n of its own set instead of inv_n
__device__ __forceinline__ void fetch_x_tile(f32x4 (&v)[NQ], const Common &C, const Span &W, int n0, float inv_n, int t, const SetCounts *rows = nullptr)
{
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const int p = t + NT * k, r = p >> 4, c4 = p & 15;
        const long long row = W.row0 + min(n0 + r, W.n_end - 1);                         // (clamped: rows beyond the range are zeroed at the store)
        const float4 xv = x_row4(C, row, c4, rows ? rows->inv((int)row) : inv_n);
        v[k] = f32x4{xv.x, xv.y, xv.z, xv.w};
    }
}
// the tile of a small input, and the columns of W1 that act on it, straight to LDS (rows beyond the workgroup's range: zero)
__device__ __forceinline__ void fill_xsmall(float (*xsmall)[DS_MAX], const Common &C, const Span &W, int n0, int t)
{
    for (int p = t; p < TM * C.d_in; p += NT) {
        const int r = p / C.d_in, c = p - r * C.d_in, n = n0 + r;
        xsmall[r][c] = n < W.n_end ? C.x[(W.row0 + n) * C.d_in + c] : 0.0f;
    }
}
__device__ __forceinline__ void fill_w1small(float (*w1small)[DS_MAX], const Common &C, int t)
{
    for (int p = t; p < HS * C.d_in; p += NT) { const int r = p / C.d_in, c = p - r * C.d_in; w1small[r][c] = C.P.W1[(long long)r * C.P.ldw1 + c]; }
}

__device__ __forceinline__ float inv_count(const Common &C)
{
    return C.mask_is_count ? 1.0f / *C.mask : (C.inv_n ? *C.inv_n : C.inv_n_host);
}
__device__ __forceinline__ float mask_of(const Common &C, int n)
{
    return !C.mask ? 1.0f : (C.mask_is_count ? (n < *C.mask ? 1.0f : 0.0f) : C.mask[n]);
}

// mask_of(n) for a row that may lie beyond the set (-> 0): no branch around the load
__device__ __forceinline__ float mask_or_zero(const Common &C, int n, int n_end)
{
    const float mk = !C.mask ? 1.0f : (C.mask_is_count ? (n < *C.mask ? 1.0f : 0.0f) : C.mask[min(n, n_end - 1)]);
    return n < n_end ? mk : 0.0f;
}

// A tile of rows of a row-major [., 64] global array as a RAW BUFFER whose size is the tile's valid rows: a store (load) to a row beyond
// them is dropped (returns 0) by the hardware's range check -- no `if (row < n_end)` around each of an epilogue's 16 stores, which
// compiled to a branch, an exec save / restore and a 64-bit address computation per store (~1000 cycles of a 4500-cycle phase).
struct RowTile {
    __amdgpu_buffer_rsrc_t r;
    __device__ __forceinline__ RowTile(const float *tile_base, int n_rows)
        : r(__builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(tile_base), 0, (n_rows > 0 ? n_rows : 0) * HS * 4, 0x00020000)) {}
    __device__ __forceinline__ void put(int row, int col, float v) const
    { __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, (row * HS + col) * 4, 0, 0); }
    // (dword accesses only: hipcc 7.2.26015 compiles __builtin_amdgcn_raw_buffer_load_b128 to ONE buffer_load_dword -- x is loaded, and y,
    //  z, w come back as COPIES OF x instead of their dwords of the source (got 1 1 1 1 5 5 5 5 for a source 1 2 3 4 5 6 7 8).  Probe:
    //  tools/probe_buffer_load_b128.hip, its MI355X output profiles/r6_probe_buffer_load_b128.txt; the ISA side of the
    //  claim is asserted without a GPU by tests/test_kernel_resources.py::test_toolchain_probes_compile)
    __device__ __forceinline__ float get(int row, int col) const
    { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (row * HS + col) * 4, 0, 0)); }
};

// the set's pooled context: pooled[k] = inv_n * sum over the producer's workgroups; cs[u] = b1[u] + W1[u][d_in + .] . pooled.
// In two halves: every load first -- the partial sums AND this thread's 16 context-column weights (thread (unit t / 4, quarter t % 4)),
// which do not depend on the sums but stood behind the barrier that publishes them: one round trip to L2 instead of two -- then the
// LDS hand-over and the product.
struct CtxLoad { float sum, b1; float w[16]; };
__device__ __forceinline__ void context_issue(const Common &C, int b, int t, CtxLoad &L)
{
    L.sum = 0.0f;
    if (C.ctx_part) {
        const int u = t >> 2, q = t & 3;
        const float *w = C.P.W1 + (long long)u * C.P.ldw1 + C.d_in + 16 * q;
#pragma unroll
        for (int k = 0; k < 16; ++k) L.w[k] = w[k];
        L.b1 = C.P.b1[u];
        if (t < HS) L.sum = sum_in_order(C.ctx_part + (long long)b * C.S_ctx * HS + t, C.S_ctx, HS);
    } else {
        L.b1 = C.P.b1[t & (HS - 1)];
    }
}
__device__ __forceinline__ void context_publish(const Common &C, float *pooled, int t, const CtxLoad &L, float inv_n)
{
    if (C.ctx_part && t < HS) pooled[t] = L.sum * inv_n;
}
__device__ __forceinline__ void context_product(const Common &C, const float *pooled, float *cs, int t, const CtxLoad &L)   // (behind a barrier)
{
    if (C.ctx_part) {
        const int u = t >> 2, q = t & 3;
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) a = fmaf(L.w[k], pooled[16 * q + k], a);
        a += __shfl_xor(a, 1);
        a += __shfl_xor(a, 2);
        if (q == 0) cs[u] = a + L.b1;
    } else if (t < HS) {
        cs[t] = L.b1;
    }
}
__device__ __forceinline__ void context(const Common &C, int b, float *pooled, float *cs, int t, float inv_n)
{
    CtxLoad L;
    context_issue(C, b, t, L);
    context_publish(C, pooled, t, L, inv_n);
    if (C.ctx_part) __syncthreads();
    context_product(C, pooled, cs, t, L);
}

// ---- the forward steps
// this wave's 32 x 32 tile of in W^T: a tile of rows against a weight matrix [unit out][unit in], both in LDS
__device__ __forceinline__ f32x16 fwd_product(const float (*in)[LD], const float (*w)[LD], const Lane &L)
{
    return mma64<1, 1>(&in[32 * L.rb + L.m][32 * L.kk], &w[L.u][32 * L.kk], zero16());
}
// a hidden layer: out = ReLU(in W^T + bias), to LDS (the next layer's input) and (SAVE: training) to global memory, saved for the
// backward; rows beyond the tile's valid ones are dropped by g's range check
template <bool SAVE = true>
__device__ __forceinline__ void relu_layer(const float (*in)[LD], const float (*w)[LD], float bias, float (*out)[LD], const RowTile &g, const Lane &L)
{
    const f32x16 acc = fwd_product(in, w, L);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int r = 32 * L.rb + drow(v, L.kk);
        const float val = fmaxf(acc[v] + bias, 0.0f);
        out[r][L.u] = val;
        if (SAVE) g.put(r, L.u, val);
    }
}
// the first hidden layer of a small input as plain FMAs (cs: bias and context): thread (unit t & 63, rows 16 (t >> 6) ...)
template <bool SAVE = true>
__device__ __forceinline__ void small_layer1(const float (*xsmall)[DS_MAX], const float (*w1small)[DS_MAX], const float *cs, int d_in,
                                             float (*out)[LD], const RowTile &g, const Lane &L)
{
    float w[DS_MAX];
#pragma unroll
    for (int c = 0; c < DS_MAX; ++c) w[c] = c < d_in ? w1small[L.uu][c] : 0.0f;
    const float c0 = cs[L.uu];
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {
        const int r = 16 * L.rg + q;
        float a = c0;
#pragma unroll
        for (int c = 0; c < DS_MAX; ++c) if (c < d_in) a = fmaf(w[c], xsmall[r][c], a);
        const float val = fmaxf(a, 0.0f);
        out[r][L.uu] = val;
        if (SAVE) g.put(r, L.uu, val);
    }
}
// the masked sums of an output over the workgroup's trials: the fixed-order sum of the four lanes that share a column
__device__ __forceinline__ void pooled_sum(float (*red)[64], float pacc, float *pool_row, const Lane &L)
{
    red[L.wave][L.lane] = pacc;
    __syncthreads();
    if (L.t < HS) {
        const int cb = L.t >> 5, n = L.t & 31;
        pool_row[L.t] = (red[cb][n] + red[cb][n + 32]) + (red[2 + cb][n] + red[2 + cb][n + 32]);
    }
}

// ------------------------------------------------------------------------------------------------ forward
struct FwdOut {
    float *h1, *h2;        // [B * N, 64] the two hidden activations (after their ReLU): saved for the backward
    float *y;              // [B * N, ldy] the output (columns [0, d_out)), or null (only its pooled sums are wanted)
    float *pool_part;      // [B, S, 64] masked sums of the output over this workgroup's trials, or null
    int ldy;               // row stride of y (>= d_out + n_extra)
    const float *extra;    // not null: columns [d_out, d_out + n_extra) of y are filled from extra[row * extra_stride + .] -- the
    int n_extra, extra_stride;   // "direct conditions" of the amortizer (log N) appended to the summary without a concatenation
};

// layer 3 (no activation) of one tile: its output rows -- and the direct conditions' columns beside them -- to y, and this thread's
// share of the masked sums of the output into pacc.  rows (see fetch_x_tile): the row of a set WITHOUT trials is NaN -- its input, a
// mean over nothing, is 0 x inf already, but the ReLUs' fmaxf gives a NaN no way through the layers, so it is written here
__device__ __forceinline__ void output_layer(const float (*in)[LD], const float (*w)[LD], float bias3, const Common &C, const FwdOut &O, const Span &W,
                                             int n0, float &pacc, const Lane &L, const SetCounts *rows = nullptr)
{
    const int u = L.u, n_end = W.n_end;
    const f32x16 acc = fwd_product(in, w, L);
    // (branch-free: y as a raw buffer of the tile's valid rows -- of NO rows if y is not wanted -- whose range check drops the
    //  stores of the other rows; a lane whose column is not written aims past the buffer; the pooled sum takes a zero mask)
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(O.y ? O.y + (W.row0 + n0) * O.ldy : O.h1, 0,
                                                                          O.y ? (n_end - n0) * O.ldy * 4 : 0, 0x00020000);
    const bool colv = u < C.d_out, cole = O.extra && !colv && u < C.d_out + O.n_extra;
    const int ue = min(max(u - C.d_out, 0), max(O.n_extra - 1, 0));
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int r = 32 * L.rb + drow(v, L.kk), n = n0 + r;
        float val = acc[v] + bias3;
        if (rows) val = rows->of((int)W.row0 + min(n, n_end - 1)) > 0 ? val : __builtin_nanf("");
        if (O.pool_part) pacc = fmaf(colv ? mask_or_zero(C, n, n_end) : 0.0f, val, pacc);
        float outv = val;
        if (O.extra) { const float e = O.extra[(W.row0 + min(n, n_end - 1)) * O.extra_stride + ue]; outv = cole ? e : val; }
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, outv), ry, (colv || cole) ? (r * O.ldy + u) * 4 : 0x7ffffff0, 0, 0);
    }
}

// One MLP over the workgroup's trials W, as the sequence of steps that both the training kernel (SAVE: h1 and h2 go to global
// memory for the backward) and the inference kernels (not SAVE: nothing but y / pool_part is written) are.  inv_n: 1 / (the set's
// number of real trials); rows: see fetch_x_tile.
template <bool BIG, bool SAVE>        // BIG: d_in == 64 (layer 1 is an MFMA product) or d_in <= DS_MAX
__device__ __forceinline__ void mlp_fwd_steps(const Common &C, const FwdOut &O, const Span &W, float inv_n, const SetCounts *rows)
{
    __shared__ __attribute__((aligned(16))) float w1s[BIG ? HS : 1][LD];
    __shared__ __attribute__((aligned(16))) float w2s[HS][LD];
    __shared__ __attribute__((aligned(16))) float w3s[HS][LD];
    __shared__ __attribute__((aligned(16))) float xs[BIG ? TM : 1][LD];
    __shared__ __attribute__((aligned(16))) float h1s[TM][LD];
    __shared__ __attribute__((aligned(16))) float h2s[TM][LD];
    __shared__ float w1small[BIG ? 1 : HS][DS_MAX], xsmall[BIG ? 1 : TM][DS_MAX];
    __shared__ float cs[HS], pooled[HS], red[4][64];
    const Lane L;
    const int t = L.t, u = L.u, n_begin = W.n_begin, n_end = W.n_end;
    STAMP(100);
    // every global load first: W1 (needed first), W2, W3 into registers; W2 and W3 go to LDS behind layers 1 and 2 (the barriers
    // that are there anyway), so their latency runs beside the input tile's, the context's and layer 1
    // (the loads complete in issue order: the input tile and W1 first, they are stored first)
    f32x4 r1[NQ], r2[NQ], r3[NQ], rx[NQ];
    if (BIG) fetch_x_tile(rx, C, W, n_begin, inv_n, t, rows);
    else fill_xsmall(xsmall, C, W, n_begin, t);
    fetch64(r1, BIG ? C.P.W1 : C.P.W2, BIG ? C.P.ldw1 : HS, t);
    fetch64(r2, C.P.W2, HS, t);
    fetch64(r3, C.P.W3, HS, t, C.d_out);
    if (BIG) {
        store_tile(xs, rx, W, n_begin, t);
        store64(w1s, r1, t);
    } else fill_w1small(w1small, C, t);
    context(C, W.b, pooled, cs, t, inv_n);
    __syncthreads();
    const float bias2 = C.P.b2[u], bias3 = u < C.d_out ? C.P.b3[u] : 0.0f, bias1 = cs[u];
    float pacc = 0.0f;
    STAMP(101);
    for (int n0 = n_begin; n0 < n_end; n0 += TM) {
        if (n0 != n_begin) {
            if (BIG) {
                fetch_x_tile(rx, C, W, n0, inv_n, t, rows);
                store_tile(xs, rx, W, n0, t);
            } else fill_xsmall(xsmall, C, W, n0, t);
            __syncthreads();
        }
        STAMP(102);
        const RowTile th1(O.h1 + (W.row0 + n0) * HS, SAVE ? n_end - n0 : 0), th2(O.h2 + (W.row0 + n0) * HS, SAVE ? n_end - n0 : 0);
        if (BIG) relu_layer<SAVE>(xs, w1s, bias1, h1s, th1, L);             // layer 1
        else small_layer1<SAVE>(xsmall, w1small, cs, C.d_in, h1s, th1, L);
        if (n0 == n_begin) store64(w2s, r2, t);      // (its first reader is layer 2, behind the barrier)
        __syncthreads();
        STAMP(103);
        relu_layer<SAVE>(h1s, w2s, bias2, h2s, th2, L);      // layer 2
        if (n0 == n_begin) store64(w3s, r3, t, C.d_out);
        __syncthreads();
        STAMP(104);
        output_layer(h2s, w3s, bias3, C, O, W, n0, pacc, L, rows);       // layer 3, and the masked sums of its output
        STAMP(105);
        // (the next tile's writes to xs / h1s / h2s are each behind a barrier every reader of this tile has passed)
    }
    if (O.pool_part) pooled_sum(red, pacc, O.pool_part + (long long)W.wg * HS, L);
}

template <bool BIG>
__global__ __launch_bounds__(NT) void mlp_fwd_kernel(Common C, FwdOut O)
{
    mlp_fwd_steps<BIG, true>(C, O, Span(C), inv_count(C), nullptr);
}

// ---- two MLPs in one launch --------------------------------------------------------------------------------------------------
// An equivariant MLP (A: input x, the set's pooled context through W1's context columns, output y) and the MLP that consumes its
// output row by row (B: the NEXT block's invariant MLP, or the pre-pooling MLP; no context; only the masked per-set sums of its
// output are wanted).  B's rows are A's rows, so nothing crosses a workgroup between them: the y tile stays in LDS as B's input,
// B's three weight matrices are fetched into registers while A computes and stored to LDS when A's readers are done -- one launch
// and one exposed weight-staging latency instead of two of each.  One 64-row tile per workgroup (rows_per_wg == TM).
// As steps over the workgroup's trials W, like mlp_fwd_steps: SAVE (training) stores both MLPs' h1 / h2 and always y; not SAVE
// (inference) only O2.pool_part, and y where O.y is not null (the next block reads it; after the last block nobody does).
template <bool BIG, bool SAVE>        // BIG, of MLP A: d_in == 64 or d_in <= DS_MAX (B's input is A's 64-wide output)
__device__ __forceinline__ void mlp2_fwd_steps(const Common &C, const FwdOut &O, const Mlp &P2, const FwdOut &O2, const Span &W, float inv_n)
{
    __shared__ __attribute__((aligned(16))) float w1s[HS][LD];
    __shared__ __attribute__((aligned(16))) float w2s[HS][LD];
    __shared__ __attribute__((aligned(16))) float w3s[HS][LD];
    __shared__ __attribute__((aligned(16))) float xs[TM][LD];
    __shared__ __attribute__((aligned(16))) float h1s[TM][LD];
    __shared__ __attribute__((aligned(16))) float h2s[TM][LD];
    __shared__ float w1small[BIG ? 1 : HS][DS_MAX], xsmall[BIG ? 1 : TM][DS_MAX];
    __shared__ float cs[HS], pooled[HS], red[4][64];
    const Lane L;
    const int t = L.t, u = L.u, n0 = W.n_begin, n_end = W.n_end;
    // ---- every global load up front, in the order of need: A's input tile and W1 (stored at once), A's W2 and W3 (stored behind
    //      A's layers 1 and 2), B's three matrices (stored when A is done)
    f32x4 r1[NQ], r2[NQ], r3[NQ], rx[NQ];
    if (BIG) fetch_x_tile(rx, C, W, n0, inv_n, t);
    else fill_xsmall(xsmall, C, W, n0, t);
    fetch64(r1, BIG ? C.P.W1 : C.P.W2, BIG ? C.P.ldw1 : HS, t);
    fetch64(r2, C.P.W2, HS, t);
    fetch64(r3, C.P.W3, HS, t);
    f32x4 q1[NQ], q2[NQ], q3[NQ];
    fetch64(q1, P2.W1, HS, t);
    fetch64(q2, P2.W2, HS, t);
    fetch64(q3, P2.W3, HS, t);
    if (BIG) {
        store_tile(xs, rx, W, n0, t);
        store64(w1s, r1, t);
    } else fill_w1small(w1small, C, t);
    context(C, W.b, pooled, cs, t, inv_n);
    __syncthreads();
    const float bias2 = C.P.b2[u], bias3 = C.P.b3[u], bias1 = cs[u];
    const float c1 = P2.b1[u], c2 = P2.b2[u], c3 = P2.b3[u];
    const int nv = n_end - n0, ns = SAVE ? nv : 0;   // the tile's valid rows: stores beyond them are dropped by the buffers' range check
    const bool want_y = SAVE || O.y != nullptr;
    const RowTile th1(O.h1 + (W.row0 + n0) * HS, ns), th2(O.h2 + (W.row0 + n0) * HS, ns), ty(O.y + (W.row0 + n0) * HS, want_y ? nv : 0);
    const RowTile tg1(O2.h1 + (W.row0 + n0) * HS, ns), tg2(O2.h2 + (W.row0 + n0) * HS, ns);
    // ---- MLP A
    if (BIG) relu_layer<SAVE>(xs, w1s, bias1, h1s, th1, L);
    else small_layer1<SAVE>(xsmall, w1small, cs, C.d_in, h1s, th1, L);
    store64(w2s, r2, t);
    __syncthreads();
    relu_layer<SAVE>(h1s, w2s, bias2, h2s, th2, L);
    store64(w3s, r3, t);
    __syncthreads();
    {   // A's output: to global memory (the next equivariant MLP and the backward read it) and into xs as B's input
        const f32x16 acc = fwd_product(h2s, w3s, L);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r = 32 * L.rb + drow(v, L.kk), n = n0 + r;
            const float val = n < n_end ? acc[v] + bias3 : 0.0f;          // (rows beyond the set: zero, as a loaded tile has them)
            xs[r][u] = val;                                               // (xs: A's layer 1 finished reading it two barriers ago)
            if (want_y) ty.put(r, u, val);
        }
    }
    __syncthreads();                                 // A's readers of w1s / w2s / w3s / h1s / h2s are done; xs is complete
    store64(w1s, q1, t);
    store64(w2s, q2, t);
    store64(w3s, q3, t);
    __syncthreads();
    // ---- MLP B
    relu_layer<SAVE>(xs, w1s, c1, h1s, tg1, L);
    __syncthreads();
    relu_layer<SAVE>(h1s, w2s, c2, h2s, tg2, L);
    __syncthreads();
    float pacc = 0.0f;
    {
        const f32x16 acc = fwd_product(h2s, w3s, L);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int n = n0 + 32 * L.rb + drow(v, L.kk);
            pacc = fmaf(mask_or_zero(C, n, n_end), acc[v] + c3, pacc);
        }
    }
    pooled_sum(red, pacc, O2.pool_part + (long long)W.wg * HS, L);
}

template <bool BIG>
__global__ __launch_bounds__(NT) void mlp2_fwd_kernel(Common C, FwdOut O, Mlp P2, FwdOut O2)
{
    mlp2_fwd_steps<BIG, true>(C, O, P2, O2, Span(C), inv_count(C));
}

// ---- inference: the whole summary network with a trial count per set (nddm_deepset_summary) -----------------------------------
// The same steps, one 64-row tile per workgroup as in training, with three differences: nothing is saved for a backward; set b's rows
// end at its own count K.of(b), so a row at or beyond it is never loaded (Common's mask stays null: every row a workgroup owns is
// real) and 1 / n is the set's own; a workgroup whose tile lies wholly beyond its set's count writes zero partial sums -- what the
// consumers add in tile order -- and is done.  For equal counts these are the training forward's sums in the training forward's
// order (there the rows beyond the count enter every sum as fmaf(0, finite, sum)).
__device__ __forceinline__ bool tile_is_empty(const Span &W, float *pool_part)
{
    if (W.n_begin < W.n_end) return false;
    if (threadIdx.x < HS) pool_part[(long long)W.wg * HS + threadIdx.x] = 0.0f;
    return true;
}
// the first pooling MLP, on the raw trials (no context): writes O.pool_part
__global__ __launch_bounds__(NT) void summary_first_kernel(Common C, FwdOut O, SetCounts K)
{
    const int b = blockIdx.x / C.S;
    const Span W(C, K.of(b));
    if (tile_is_empty(W, O.pool_part)) return;
    mlp_fwd_steps<false, false>(C, O, W, K.inv(b), nullptr);
}
// an equivariant MLP and the pooling MLP on its output: writes O2.pool_part, and O.y where the next block wants it
template <bool BIG>
__global__ __launch_bounds__(NT) void summary_pair_kernel(Common C, FwdOut O, Mlp P2, FwdOut O2, SetCounts K)
{
    const int b = blockIdx.x / C.S;
    const Span W(C, K.of(b));
    if (tile_is_empty(W, O2.pool_part)) return;
    mlp2_fwd_steps<BIG, false>(C, O, P2, O2, W, K.inv(b));
}
// the MLP after the pooling, launched over the B pooled rows as ONE "set": row r is the mean of set r, by set r's own count
__global__ __launch_bounds__(NT) void summary_post_kernel(Common C, FwdOut O, SetCounts K)
{
    mlp_fwd_steps<true, false>(C, O, Span(C), 0.0f, &K);
}

// ------------------------------------------------------------------------------------------------ backward
// The gradient of a pooled output per unit of the set, gp[k] = inv_n * sum_i gp_W[i][k] * (sum over the consumer's workgroups of gpool[.][i]),
// in the same two halves as the context: the partial sums and this thread's 16 weights (thread (unit t / 4, quarter t % 4)) in one round trip.
struct GpLoad { float sum; float w[16]; };
__device__ __forceinline__ void gp_issue(const float *gpool, int gp_S, const float *gp_W, int gp_ldw, int b, int t, GpLoad &L)
{
    const int k = t >> 2, q = t & 3;
#pragma unroll
    for (int i = 0; i < 16; ++i) L.w[i] = gp_W[(long long)(16 * q + i) * gp_ldw + k];
    L.sum = t < HS ? sum_in_order(gpool + (long long)b * gp_S * HS + t, gp_S, HS) : 0.0f;
}
__device__ __forceinline__ void gp_product(const float *dsum, float *gp, float inv_n, int t, const GpLoad &L)      // (behind a barrier)
{
    const int k = t >> 2, q = t & 3;
    float a = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) a = fmaf(L.w[i], dsum[16 * q + i], a);
    a += __shfl_xor(a, 1);
    a += __shfl_xor(a, 2);
    if (q == 0) gp[k] = a * inv_n;
}

// ---- the backward steps.  g: d(pre-activation) of a layer's output, h: the layer's input, both tiles in LDS
// what a thread accumulates of one MLP's weight gradients: its registers of the three products g^T h (tile (rb, ub): row = unit out,
// column = unit in), and as thread (unit t & 63, rows 16 (t >> 6) ..) the column sums of d(pre-activation 1..3) and (a small
// input) row t & 63 of dW1 over the same rows
struct Grads {
    f32x16 aW1, aW2, aW3;
    float db[3], dw1[DS_MAX];
    __device__ __forceinline__ Grads() : aW1(zero16()), aW2(zero16()), aW3(zero16()), db{0.0f, 0.0f, 0.0f}, dw1{0.0f, 0.0f, 0.0f, 0.0f} {}
};
// dW [unit out, unit in] += g^T h (the k's are the tile's rows)
__device__ __forceinline__ f32x16 wgrad(const float (*g)[LD], const float (*h)[LD], f32x16 aW, const Lane &L)
{
    return mma64<LD, LD>(&g[32 * L.kk][32 * L.rb + L.m], &h[32 * L.kk][L.u], aW);
}
// db += the column sums of g
__device__ __forceinline__ void bias_grad(const float (*g)[LD], float &db, const Lane &L)
{
#pragma unroll 8
    for (int q = 0; q < 16; ++q) db += g[16 * L.rg + q][L.uu];
}
// d h = g W (w [unit out][unit in])
__device__ __forceinline__ f32x16 dgrad(const float (*g)[LD], const float (*w)[LD], const Lane &L)
{
    return mma64<1, LD>(&g[32 * L.rb + L.m][32 * L.kk], &w[32 * L.kk][L.u], zero16());
}
// a hidden layer, whose input h is the ReLU output of the layer before: dW, db, and out = that layer's d(pre-activation).
// (out is never a tile this step reads: every reader of its old content finished before the barrier in front of the step)
__device__ __forceinline__ void bwd_layer(const float (*g)[LD], const float (*h)[LD], const float (*w)[LD], float (*out)[LD], f32x16 &aW, float &db,
                                          const Lane &L)
{
    aW = wgrad(g, h, aW, L);
    bias_grad(g, db, L);
    const f32x16 acc = dgrad(g, w, L);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int r = 32 * L.rb + drow(v, L.kk);
        out[r][L.u] = h[r][L.u] > 0.0f ? acc[v] : 0.0f;
    }
}
// dW1 of a small input as plain FMAs, g = d(pre-activation 1)
__device__ __forceinline__ void small_dw1(const float (*g)[LD], const float (*xsmall)[DS_MAX], int d_in, float (&dw1)[DS_MAX], const Lane &L)
{
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {
        const float d = g[16 * L.rg + q][L.uu];
#pragma unroll
        for (int c = 0; c < DS_MAX; ++c) if (c < d_in) dw1[c] = fmaf(d, xsmall[16 * L.rg + q][c], dw1[c]);
    }
}
// this workgroup's partial sums of one MLP's weight gradients -> wp (its row of wpart: W1 [64, ld1], b1, W2, b2, W3 [d_out, 64], b3).
// dctx_part: not null: the column sums of d(pre-activation 1) also go to this workgroup's row of it; ctx_cols: W1 has context columns
// [d_in, d_in + 64), whose gradient is those sums x pooled.  (Behind its first barrier every reader of the MLP's tiles is done.)
template <bool BIG>
__device__ __forceinline__ void wgrad_epilogue(float *wp, int ld1, int d_in, int d_out, const Grads &G, float (*red)[3][HS], float (*redw)[HS][DS_MAX],
                                               float *db1s, float *dctx_part, bool ctx_cols, const float *pooled, const Span &W, const Lane &L)
{
    const int t = L.t, oW1 = 0, ob1 = HS * ld1, oW2 = ob1 + HS, ob2 = oW2 + HS * HS, oW3 = ob2 + HS, ob3 = oW3 + d_out * HS;
    const RowTile tw3(wp + oW3, d_out);
#pragma unroll
    for (int v = 0; v < 16; ++v) {                   // tile (rb, ub): row = unit out, column = unit in
        const int r = 32 * L.rb + drow(v, L.kk);
        wp[oW2 + r * HS + L.u] = G.aW2[v];
        tw3.put(r, L.u, G.aW3[v]);                   // (rows >= d_out: dropped)
        if (BIG) wp[oW1 + r * ld1 + L.u] = G.aW1[v];
    }
#pragma unroll
    for (int l = 0; l < 3; ++l) red[L.rg][l][L.uu] = G.db[l];
    if (!BIG) {
#pragma unroll
        for (int c = 0; c < DS_MAX; ++c) redw[L.rg][L.uu][c] = G.dw1[c];
    }
    __syncthreads();
    if (t < 3 * HS) {
        const int l = t >> 6, c = t & 63;
        const float v = (red[0][l][c] + red[1][l][c]) + (red[2][l][c] + red[3][l][c]);
        if (l < 2 || c < d_out) wp[l == 0 ? ob1 + c : (l == 1 ? ob2 + c : ob3 + c)] = v;
        if (l == 0) {
            db1s[c] = v;
            if (dctx_part) dctx_part[(long long)W.wg * HS + c] = v;
        }
    }
    if (!BIG && t < HS)
        for (int c = 0; c < d_in; ++c) wp[oW1 + t * ld1 + c] = (redw[0][t][c] + redw[1][t][c]) + (redw[2][t][c] + redw[3][t][c]);
    if (ctx_cols) {                                  // context columns of W1: (sum of d pre-activation 1) x pooled
        __syncthreads();
        for (int p = t; p < HS * HS; p += NT) {
            const int r = p >> 6, k = p & 63;
            wp[oW1 + r * ld1 + d_in + k] = db1s[r] * pooled[k];
        }
    }
}

struct BwdIO {
    const float *h1, *h2;            // saved by the forward
    const float *gy; int ldgy;       // [B * N, ldgy] gradient of the output (columns [0, d_out)), or null
    const float *gpool; int gp_S;    // gradient through the pooled output (null: none), one of two forms:
    const float *gp_W; int gp_ldw;   //   gp_W != null: gpool [B, gp_S, 64] = the consumer's per-workgroup sums of d(pre-activation 1),
                                     //     to be taken through the consumer's context columns gp_W [64, gp_ldw] and 1 / n;
                                     //   gp_W == null: gpool [B, 64] = the gradient of the masked MEAN (1 / n is applied here)
    float *gx; int gx_acc;           // [B * N, d_in] gradient of the input, or null; gx_acc: add to what it holds
    float *dctx_part;                // [B, S, 64] this workgroup's sum of d(pre-activation 1) (the context's gradient), or null
    float *wpart; int ld_part;       // row blockIdx.x (stride ld_part floats) takes this workgroup's weight gradients:
                                     // W1 [64, ldw1], b1, W2, b2, W3, b3
};

// fetch_tile of the output's gradient (null: zeros; store_tile stores it)
__device__ __forceinline__ void fetch_gy_tile(f32x4 (&v)[NQ], const float *gy, int ldgy, int d_out, const Span &W, int n0, int t)
{
    if (!gy) {
#pragma unroll
        for (int k = 0; k < NQ; ++k) v[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    } else if (d_out == HS && ldgy == HS) fetch_tile(v, gy, W, n0, t);
    else {                                           // a narrow output (the summary): columns < d_out, rows ldgy floats apart
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            const int p = t + NT * k, r = p >> 4, c4 = p & 15, cl = d_out - 1;
            const float *gr = gy + (W.row0 + min(n0 + r, W.n_end - 1)) * ldgy;
            const float a0 = gr[min(4 * c4, cl)], a1 = gr[min(4 * c4 + 1, cl)], a2 = gr[min(4 * c4 + 2, cl)], a3 = gr[min(4 * c4 + 3, cl)];
            v[k] = f32x4{4 * c4 < d_out ? a0 : 0.0f, 4 * c4 + 1 < d_out ? a1 : 0.0f, 4 * c4 + 2 < d_out ? a2 : 0.0f, 4 * c4 + 3 < d_out ? a3 : 0.0f};
        }
    }
}

template <bool BIG>
__global__ __launch_bounds__(NT) void mlp_bwd_kernel(Common C, BwdIO Q)
{
    __shared__ __attribute__((aligned(16))) float w1s[BIG ? HS : 1][LD];
    __shared__ __attribute__((aligned(16))) float w2s[HS][LD];
    __shared__ __attribute__((aligned(16))) float w3s[HS][LD];
    __shared__ __attribute__((aligned(16))) float xs[BIG ? TM : 1][LD];
    __shared__ __attribute__((aligned(16))) float h1s[TM][LD];
    __shared__ __attribute__((aligned(16))) float h2s[TM][LD];
    __shared__ __attribute__((aligned(16))) float gs[TM][LD];        // gradient of the output; later d(pre-activation 1)
    __shared__ __attribute__((aligned(16))) float d2s[TM][LD];       // d(pre-activation 2)
    __shared__ float xsmall[BIG ? 1 : TM][DS_MAX];
    __shared__ float pooled[HS], cs[HS], gp[HS], dsum[HS], red[4][3][HS], redw[BIG ? 1 : 4][HS][DS_MAX], db1s[HS];
    const Lane L;
    const Span W(C);
    const int t = L.t, u = L.u, b = W.b, n_begin = W.n_begin, n_end = W.n_end;
    const float inv_n = inv_count(C);
    STAMP(200);
    auto load_tile = [&](const int n0) {             // saved activations, input and output gradient (the pooled part: added below)
        // every load unconditional, from a clamped row (rows beyond the set are zeroed at the store), and ALL of them issued before
        // the first store: inside `if (n < n_end)` each of the four passes was a branch and a round trip to L2 of its own
        f32x4 v1[NQ], v2[NQ], vg[NQ], vx[NQ];
        fetch_tile(v1, Q.h1, W, n0, t);
        fetch_tile(v2, Q.h2, W, n0, t);
        fetch_gy_tile(vg, Q.gy, Q.ldgy, C.d_out, W, n0, t);
        if (BIG) fetch_x_tile(vx, C, W, n0, inv_n, t);
        store_tile(h1s, v1, W, n0, t);
        store_tile(h2s, v2, W, n0, t);
        store_tile(gs, vg, W, n0, t);
        if (BIG) store_tile(xs, vx, W, n0, t);
        else fill_xsmall(xsmall, C, W, n0, t);
    };
    // the small loads that feed the context and the pooled gradient go FIRST (loads return in issue order): they are back while the
    // tiles and the weights are still on their way
    CtxLoad Lc;
    GpLoad Lg;
    const bool gpw = Q.gpool && Q.gp_W;
    context_issue(C, b, t, Lc);
    if (gpw) gp_issue(Q.gpool, Q.gp_S, Q.gp_W, Q.gp_ldw, b, t, Lg);
    {   // every weight load in flight before the first store (fetch, store, fetch, store ... waited for three load latencies in turn)
        f32x4 r1[NQ], r2[NQ], r3[NQ];
        fetch64(r3, C.P.W3, HS, t, C.d_out);
        fetch64(r2, C.P.W2, HS, t);
        fetch64(r1, BIG ? C.P.W1 : C.P.W2, BIG ? C.P.ldw1 : HS, t);
        load_tile(n_begin);
        store64(w3s, r3, t, C.d_out);
        store64(w2s, r2, t);
        if (BIG && Q.gx) store64(w1s, r1, t);
    }
    context_publish(C, pooled, t, Lc, inv_n);        // (pooled: also for the context columns' weight gradient)
    if (gpw && t < HS) dsum[t] = Lg.sum;
    __syncthreads();
    context_product(C, pooled, cs, t, Lc);
    if (gpw) gp_product(dsum, gp, inv_n, t, Lg);     // gradient of the pooled output, per unit of this set
    else if (Q.gpool && t < HS) gp[t] = Q.gpool[(long long)b * HS + t] * inv_n;
    __syncthreads();
    Grads G;
    for (int n0 = n_begin; n0 < n_end; n0 += TM) {
        if (n0 != n_begin) {
            __syncthreads();                         // the previous tile's readers are done
            load_tile(n0);
        }
        STAMP(201);
        if (Q.gpool) {                               // the pooled output's gradient, spread over the set's real trials
            if (n0 != n_begin) __syncthreads();
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                const int p = t + NT * k, r = p >> 4, c4 = p & 15, n = n0 + r;
                if (n < n_end) {
                    const float mk = mask_of(C, n);
                    float4 vg = *reinterpret_cast<float4 *>(&gs[r][4 * c4]);
                    vg.x = fmaf(mk, gp[4 * c4], vg.x); vg.y = fmaf(mk, gp[4 * c4 + 1], vg.y);
                    vg.z = fmaf(mk, gp[4 * c4 + 2], vg.z); vg.w = fmaf(mk, gp[4 * c4 + 3], vg.w);
                    *reinterpret_cast<float4 *>(&gs[r][4 * c4]) = vg;
                }
            }
        }
        __syncthreads();
        STAMP(202);
        bwd_layer(gs, h2s, w3s, d2s, G.aW3, G.db[2], L);             // layer 3: gs -> d(pre-activation 2) in d2s
        __syncthreads();
        STAMP(203);
        bwd_layer(d2s, h1s, w2s, gs, G.aW2, G.db[1], L);             // layer 2: d2s -> d(pre-activation 1) in gs
        __syncthreads();
        STAMP(204);
        bias_grad(gs, G.db[0], L);                                   // layer 1
        if (BIG) {
            G.aW1 = wgrad(gs, xs, G.aW1, L);
            if (Q.gx) {
                const f32x16 acc = dgrad(gs, w1s, L);
                const RowTile tgx(Q.gx + (W.row0 + n0) * HS, n_end - n0);    // (rows beyond the set: the range check drops them)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int r = 32 * L.rb + drow(v, L.kk);
                    tgx.put(r, u, Q.gx_acc ? tgx.get(r, u) + acc[v] : acc[v]);
                }
            }
        } else small_dw1(gs, xsmall, C.d_in, G.dw1, L);
    }
    STAMP(205);
    wgrad_epilogue<BIG>(Q.wpart + (long long)W.wg * Q.ld_part, C.P.ldw1, C.d_in, C.d_out, G, red, redw, db1s, Q.dctx_part, C.ctx_part != nullptr, pooled,
                        W, L);
    STAMP(206);
}

// ---- two MLPs' backward in one launch --------------------------------------------------------------------------------------------
// The mirror image of mlp2_fwd_kernel: the backward of a POOLING MLP X (the next block's invariant MLP or the pre-pooling MLP: its
// output gradient arrives through the pooled mean only; its input is the output of ...) followed by the backward of the
// EQUIVARIANT MLP Y that produced that input.  X's input gradient -- plus, where the rows also fed an equivariant MLP, that MLP's
// input gradient from the launch before (gx_prev) -- is Y's output gradient, row for row: it stays in LDS.  Y's weights, saved
// activations and input tile are fetched into registers while X computes.  Common describes Y.  One tile per workgroup.
struct Bwd2 {
    const float *x1;                 // [B * N, 64] X's input (= Y's output, saved by the forward)
    Mlp PX;                          // X's weights (no context: W1 [64, 64])
    const float *h1x, *h2x;          // X's saved activations
    const float *gpool; int gp_S;    // the gradient through X's pooled output: the two forms of BwdIO
    const float *gp_W; int gp_ldw;
    const float *gx_prev;            // [B * N, 64] or null: added to X's input gradient
    float *wpart_x;                  // X's weight-gradient partial sums (row blockIdx.x, stride ld_part)
    const float *h1y, *h2y;          // Y's saved activations
    float *gx;                       // [B * N, 64] Y's input gradient, or null (always null for a small input)
    float *dctx_part;                // [B, S, 64] Y's sum of d(pre-activation 1)
    float *wpart_y; int ld_part;
};

template <bool BIG>        // of Y: d_in == 64 or d_in <= DS_MAX
// (143 KB of LDS: one workgroup per CU, i.e. one wave per SIMD -- the whole register file is this wave's; with the default
//  budget the prefetched operands spilled to scratch)
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(1, 1))) void mlp2_bwd_kernel(Common C, Bwd2 Q)
{
    __shared__ __attribute__((aligned(16))) float w1s[HS][LD];
    __shared__ __attribute__((aligned(16))) float w2s[HS][LD];
    __shared__ __attribute__((aligned(16))) float w3s[HS][LD];
    __shared__ __attribute__((aligned(16))) float xs[TM][LD];
    __shared__ __attribute__((aligned(16))) float h1s[TM][LD];
    __shared__ __attribute__((aligned(16))) float h2s[TM][LD];
    __shared__ __attribute__((aligned(16))) float gs[TM][LD];
    __shared__ __attribute__((aligned(16))) float d2s[TM][LD];
    __shared__ float xsmall[BIG ? 1 : TM][DS_MAX];
    __shared__ float pooled[HS], cs[HS], gp[HS], dsum[HS], red[4][3][HS], redw[BIG ? 1 : 4][HS][DS_MAX], db1s[HS];
    const Lane L;
    const Span W(C);
    const int t = L.t, u = L.u, b = W.b, n0 = W.n_begin, n_end = W.n_end;
    const float inv_n = inv_count(C);
    // ---- Y's pooled context and the gradient of X's pooled output, per unit of this set: their loads go out FIRST and are consumed
    //      before the operand fetches below are issued (this kernel has no registers left to hold both) -- behind those fetches,
    //      in issue order, they cost four round trips at the head of the kernel
    {
        CtxLoad Lc;
        GpLoad Lg;
        context_issue(C, b, t, Lc);
        if (Q.gp_W) gp_issue(Q.gpool, Q.gp_S, Q.gp_W, Q.gp_ldw, b, t, Lg);
        context_publish(C, pooled, t, Lc, inv_n);
        if (Q.gp_W && t < HS) dsum[t] = Lg.sum;
        __syncthreads();
        context_product(C, pooled, cs, t, Lc);
        if (Q.gp_W) gp_product(dsum, gp, inv_n, t, Lg);
        else if (t < HS) gp[t] = Q.gpool[(long long)b * HS + t] * inv_n;
    }
    // ---- every global load up front, in the order of need.  X: h2 and W3 (layer 3 runs first), then h1 and W2, then the input tile
    //      and W1; they are stored to LDS just before the phase that reads them (behind the barriers that are there anyway), so
    //      one load latency is exposed instead of one per operand.  Y's operands follow and stay in registers until X is done.
    f32x4 xh2[NQ], xw3[NQ], xh1[NQ], xw2[NQ], xx[NQ], xw1[NQ];
    fetch_tile(xh2, Q.h2x, W, n0, t);
    fetch64(xw3, Q.PX.W3, HS, t);
    fetch_tile(xh1, Q.h1x, W, n0, t);
    fetch64(xw2, Q.PX.W2, HS, t);
    fetch_tile(xx, Q.x1, W, n0, t);
    fetch64(xw1, Q.PX.W1, HS, t);
    // ---- Y's operands -> registers (stored to LDS when X's readers are done)
    f32x4 q1[NQ], q2[NQ], q3[NQ], th1[NQ], th2[NQ], tx[NQ];
    fetch64(q2, C.P.W2, HS, t);
    fetch64(q3, C.P.W3, HS, t);
    fetch64(q1, BIG ? C.P.W1 : C.P.W2, BIG ? C.P.ldw1 : HS, t);          // (unconditional: a guarded fetch is a branch around every load)
    fetch_tile(th1, Q.h1y, W, n0, t);
    fetch_tile(th2, Q.h2y, W, n0, t);
    if (BIG) fetch_tile(tx, C.x, W, n0, t);
    else {
#pragma unroll
        for (int k = 0; k < NQ; ++k) tx[k] = th1[k];
        fill_xsmall(xsmall, C, W, n0, t);
    }
    // (Y's pooled context and the gradient of X's pooled output were computed at the head of the kernel: see there)
    store_tile(h2s, xh2, W, n0, t);
    store64(w3s, xw3, t);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NQ; ++k) {                   // the pooled output's gradient, spread over the set's real trials (rows beyond: zero)
        const int p = t + NT * k, r = p >> 4, c4 = p & 15, n = n0 + r;
        const float mk = n < n_end ? mask_of(C, n) : 0.0f;
        *reinterpret_cast<float4 *>(&gs[r][4 * c4]) = make_float4(mk * gp[4 * c4], mk * gp[4 * c4 + 1], mk * gp[4 * c4 + 2], mk * gp[4 * c4 + 3]);
    }
    __syncthreads();
    // ================================================================================ X
    {
        Grads G;
        bwd_layer(gs, h2s, w3s, d2s, G.aW3, G.db[2], L);
        store_tile(h1s, xh1, W, n0, t);              // (layer 2's operands: first read behind the barrier)
        store64(w2s, xw2, t);
        __syncthreads();
        bwd_layer(d2s, h1s, w2s, gs, G.aW2, G.db[1], L);
        store_tile(xs, xx, W, n0, t);                // (layer 1's)
        store64(w1s, xw1, t);
        __syncthreads();
        bias_grad(gs, G.db[0], L);
        G.aW1 = wgrad(gs, xs, G.aW1, L);
        {   // X's input gradient (+ the other consumer's) = Y's output gradient: into d2s (its readers finished before the barrier above)
            const f32x16 acc = dgrad(gs, w1s, L);
            const RowTile tprev(Q.gx_prev ? Q.gx_prev + (W.row0 + n0) * HS : Q.h1y, Q.gx_prev ? n_end - n0 : 0);   // (no such gradient: a buffer of no rows reads zeros)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int r = 32 * L.rb + drow(v, L.kk), n = n0 + r;
                const float g = tprev.get(r, u) + acc[v];
                d2s[r][u] = n < n_end ? g : 0.0f;
            }
        }
        // (no context, W1 [64, 64]; behind the epilogue's barrier every reader of X's tiles and weights is done and d2s is complete)
        wgrad_epilogue<true>(Q.wpart_x + (long long)W.wg * Q.ld_part, HS, HS, HS, G, red, redw, db1s, nullptr, false, pooled, W, L);
    }
    // ================================================================================ Y
    store64(w2s, q2, t);
    store64(w3s, q3, t);
    if (BIG) store64(w1s, q1, t);
    store_tile(h1s, th1, W, n0, t);
    store_tile(h2s, th2, W, n0, t);
    if (BIG) store_tile(xs, tx, W, n0, t);
    __syncthreads();                                 // (and the readers of red[] above are done before Y's epilogue writes it)
    {
        Grads G;
        // the output gradient is in d2s; gs takes d(pre-activation 2), then d2s d(pre-activation 1): the single kernel's roles, swapped
        bwd_layer(d2s, h2s, w3s, gs, G.aW3, G.db[2], L);
        __syncthreads();
        bwd_layer(gs, h1s, w2s, d2s, G.aW2, G.db[1], L);
        __syncthreads();
        bias_grad(d2s, G.db[0], L);
        if (BIG) {
            G.aW1 = wgrad(d2s, xs, G.aW1, L);
            if (Q.gx) {
                const f32x16 acc = dgrad(d2s, w1s, L);
                const RowTile tgx(Q.gx + (W.row0 + n0) * HS, n_end - n0);
#pragma unroll
                for (int v = 0; v < 16; ++v) tgx.put(32 * L.rb + drow(v, L.kk), u, acc[v]);
            }
        } else small_dw1(d2s, xsmall, C.d_in, G.dw1, L);
        wgrad_epilogue<BIG>(Q.wpart_y + (long long)W.wg * Q.ld_part, C.P.ldw1, C.d_in, HS, G, red, redw, db1s, Q.dctx_part, true, pooled, W, L);
    }
}

// out[p] = sum over g of part[g][p], g in fixed order; entries p >= P_main were written by the first G_tail rows only.
// A workgroup takes 64 columns; wave q sums the rows g = q (mod 4) of its columns (eight loads in flight per lane) -- the four sums
// a_q the one-thread-per-column form kept in four accumulators -- and wave 0 adds them as that form did: (a0 + a1) + (a2 + a3), the
// rows past the last whole group of four going to a0.  Same bits, four times the workgroups and a quarter of the dependent chain.
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float *part, int G, int P, int P_main, int G_tail, float *out)
{
    __shared__ float red[4][64];
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6, p = blockIdx.x * 64 + c, pc = min(p, P - 1);
    if (pc >= P_main) G = G_tail;
    const int G4 = G & ~3;
    const float *src = part + pc;
    float a = 0.0f;
    int g = q;
    for (; g + 28 < G4; g += 32) {                       // eight rows of this wave's residue class: the loads first, then the adds in order
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = src[(long long)(g + 4 * k) * P];
#pragma unroll
        for (int k = 0; k < 8; ++k) a += v[k];
    }
    for (; g < G4; g += 4) a += src[(long long)g * P];
    if (q == 0) for (g = G4; g < G; ++g) a += src[(long long)g * P];
    red[q][c] = a;
    __syncthreads();
    if (q == 0 && p < P) out[p] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

}  // namespace nddm_deepset

using namespace nddm_deepset;

// the 22 leading arguments of the four MLP entry points, in their order
static Common make_common(const float *x, int d_in, int B, int N, int S, int rows_per_wg, const float *mask, int mask_is_count, const float *inv_n,
                          float inv_n_host, const float *ctx_part, int S_ctx, const float *W1, int ldw1, const float *b1, const float *W2,
                          const float *b2, const float *W3, const float *b3, int d_out, const float *x_part, int S_x)
{
    return {x, d_in, B, N, S, rows_per_wg, mask, mask && mask_is_count, inv_n, inv_n_host, ctx_part, S_ctx, {W1, ldw1, b1, W2, b2, W3, b3}, d_out, x_part, S_x};
}

// one workgroup per (set, workgroup of the set): the kernel for a 64-wide input or the one for a small input.  0, or 2: the launch failed
template <typename K, typename... A>
static int launch_by_d_in(K big, K small, const Common &C, void *stream, const A &...args)
{
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (C.d_in == HS) hipLaunchKernelGGL(big, dim3(C.B * C.S), dim3(NT), 0, st, C, args...);
    else hipLaunchKernelGGL(small, dim3(C.B * C.S), dim3(NT), 0, st, C, args...);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

extern "C" {

int nddm_deepset_supported(int hidden, int d_in) { return (hidden == HS && (d_in == HS || (d_in >= 1 && d_in <= DS_MAX))) ? 1 : 0; }

static bool common_ok(const Common &C)
{
    return nddm_deepset_supported(HS, C.d_in) && C.B > 0 && C.N > 0 && C.S > 0 && C.rows_per_wg > 0 && (long long)C.S * C.rows_per_wg >= C.N
           && C.P.ldw1 == C.d_in + (C.ctx_part ? HS : 0) && (C.d_in != HS || C.P.ldw1 % 4 == 0) && C.d_out >= 1 && C.d_out <= HS
           && (C.x_part ? (C.d_in == HS && C.S_x >= 1) : C.x != nullptr);
}

/* One per-trial MLP forward.  x [B * N, d_in]; W1 [64, d_in (+ 64 with a context)], W2, W3 [64, 64]; mask [N] or NULL; inv_n: device
 * scalar or NULL (then inv_n_host); ctx_part [B, S_ctx, 64] or NULL.  Writes h1, h2 [B * N, 64], and y [B * N, 64] and / or
 * pool_part [B, S, 64] where not NULL.  S workgroups of up to rows_per_wg trials per set.  d_out: rows of W3 / b3 and width of y
 * (64 but for the last MLP of the network); x_part / S_x: see Common (NULL / 0: x is read).  ldy: row stride of y (0: d_out);
 * extra / n_extra / extra_stride: columns [d_out, d_out + n_extra) of y are copied from extra[row * extra_stride + .] (NULL: none). */
int nddm_deepset_mlp_fwd(const float *x, int d_in, int B, int N, int S, int rows_per_wg, const float *mask, int mask_is_count, const float *inv_n,
                         float inv_n_host, const float *ctx_part, int S_ctx, const float *W1, int ldw1, const float *b1, const float *W2,
                         const float *b2, const float *W3, const float *b3, int d_out, const float *x_part, int S_x, float *h1, float *h2,
                         float *y, float *pool_part, int ldy, const float *extra, int n_extra, int extra_stride, void *stream)
{
    const Common C = make_common(x, d_in, B, N, S, rows_per_wg, mask, mask_is_count, inv_n, inv_n_host, ctx_part, S_ctx, W1, ldw1, b1, W2, b2, W3, b3, d_out, x_part, S_x);
    if (ldy <= 0) ldy = d_out;
    if (!common_ok(C) || !h1 || !h2 || (pool_part && d_out != HS) || n_extra < 0 || (extra && (!y || d_out + n_extra > HS)) || ldy < d_out + (extra ? n_extra : 0))
        return 1;
    const FwdOut O = {h1, h2, y, pool_part, ldy, extra, extra ? n_extra : 0, extra_stride};
    return launch_by_d_in(mlp_fwd_kernel<true>, mlp_fwd_kernel<false>, C, stream, O);
}

/* The backward of nddm_deepset_mlp_fwd (same first arguments).  gy [B * N, 64] or NULL; gpool / gp_S / gp_W / gp_ldw: see BwdIO;
 * (ldgy: its row stride, 0: d_out); gx [B * N, d_in] or NULL (d_in == 64 only), gx_acc: accumulate; dctx_part [B, S, 64] or NULL; wpart: B * S rows, ld_part floats
 * apart, of 64 ldw1 + 64 + 2 (4096 + 64) weight-gradient partial sums each: reduce with nddm_deepset_reduce. */
int nddm_deepset_mlp_bwd(const float *x, int d_in, int B, int N, int S, int rows_per_wg, const float *mask, int mask_is_count, const float *inv_n,
                         float inv_n_host, const float *ctx_part, int S_ctx, const float *W1, int ldw1, const float *b1, const float *W2,
                         const float *b2, const float *W3, const float *b3, int d_out, const float *x_part, int S_x, const float *h1,
                         const float *h2, const float *gy, int ldgy, const float *gpool, int gp_S, const float *gp_W, int gp_ldw, float *gx,
                         int gx_acc, float *dctx_part, float *wpart, int ld_part, void *stream)
{
    if (ldgy <= 0) ldgy = d_out;
    const Common C = make_common(x, d_in, B, N, S, rows_per_wg, mask, mask_is_count, inv_n, inv_n_host, ctx_part, S_ctx, W1, ldw1, b1, W2, b2, W3, b3, d_out, x_part, S_x);
    if (!common_ok(C) || !h1 || !h2 || !wpart || ld_part < HS * ldw1 + HS + HS * HS + HS + d_out * HS + d_out || (gx && d_in != HS)
        || (!gy && !gpool) || (gpool && d_out != HS) || ldgy < d_out)
        return 1;
    const BwdIO Q = {h1, h2, gy, ldgy, gpool, gp_S, gp_W, gp_ldw, gx, gx_acc, dctx_part, wpart, ld_part};
    return launch_by_d_in(mlp_bwd_kernel<true>, mlp_bwd_kernel<false>, C, stream, Q);
}

/* nddm_deepset_mlp_fwd for an equivariant MLP A (same first arguments; d_out 64, y required) FOLLOWED IN THE SAME LAUNCH by the
 * MLP B that consumes A's output row by row (no context, input width 64; W1b, W2b, W3b [64, 64]): writes B's h1b, h2b [B * N, 64] and
 * the masked sums of B's output pool_part_b [B, S, 64] -- what two calls (A with y, then B on y with pool_part) write, bit for bit.
 * rows_per_wg must be 64 (one tile per workgroup). */
int nddm_deepset_mlp2_fwd(const float *x, int d_in, int B, int N, int S, int rows_per_wg, const float *mask, int mask_is_count, const float *inv_n,
                          float inv_n_host, const float *ctx_part, int S_ctx, const float *W1, int ldw1, const float *b1, const float *W2,
                          const float *b2, const float *W3, const float *b3, int d_out, const float *x_part, int S_x, float *h1, float *h2,
                          float *y, const float *W1b, const float *b1b, const float *W2b, const float *b2b, const float *W3b, const float *b3b,
                          float *h1b, float *h2b, float *pool_part_b, void *stream)
{
    const Common C = make_common(x, d_in, B, N, S, rows_per_wg, mask, mask_is_count, inv_n, inv_n_host, ctx_part, S_ctx, W1, ldw1, b1, W2, b2, W3, b3, d_out, x_part, S_x);
    if (!common_ok(C) || rows_per_wg != TM || d_out != HS || x_part || !h1 || !h2 || !y || !W1b || !b1b || !W2b || !b2b || !W3b || !b3b || !h1b || !h2b
        || !pool_part_b)
        return 1;
    const FwdOut O = {h1, h2, y, nullptr, HS, nullptr, 0, 0}, O2 = {h1b, h2b, nullptr, pool_part_b, HS, nullptr, 0, 0};
    const Mlp P2 = {W1b, HS, b1b, W2b, b2b, W3b, b3b};
    return launch_by_d_in(mlp2_fwd_kernel<true>, mlp2_fwd_kernel<false>, C, stream, O, P2, O2);
}

/* The backward of nddm_deepset_mlp2_fwd's pair, in the backward's order: first the pooling MLP X (input x1 [B * N, 64] = Y's output;
 * weights W1x .. b3x, all [64, 64]; saved h1x, h2x; output gradient through its pooled mean: gpool / gp_S / gp_W / gp_ldw as in
 * nddm_deepset_mlp_bwd; gx_prev [B * N, 64] or NULL is added to its input gradient), then the equivariant MLP Y (the first
 * arguments, as nddm_deepset_mlp_bwd: its input x, context ctx_part, weights; saved h1y, h2y) whose output gradient IS that input
 * gradient (it never leaves the chip).  Writes Y's gx [B * N, 64] (or NULL; must be NULL for a small input), dctx_part [B, S, 64] and
 * both MLPs' weight-gradient partial sums (rows of ld_part floats, one per workgroup) -- what the two separate calls write, bit for
 * bit.  rows_per_wg must be 64. */
int nddm_deepset_mlp2_bwd(const float *x, int d_in, int B, int N, int S, int rows_per_wg, const float *mask, int mask_is_count, const float *inv_n,
                          float inv_n_host, const float *ctx_part, int S_ctx, const float *W1, int ldw1, const float *b1, const float *W2,
                          const float *b2, const float *W3, const float *b3, int d_out, const float *x_part, int S_x, const float *h1y,
                          const float *h2y, float *gx, float *dctx_part, float *wpart_y, const float *x1, const float *W1x, const float *b1x,
                          const float *W2x, const float *b2x, const float *W3x, const float *b3x, const float *h1x, const float *h2x,
                          const float *gpool, int gp_S, const float *gp_W, int gp_ldw, const float *gx_prev, float *wpart_x, int ld_part,
                          void *stream)
{
    const Common C = make_common(x, d_in, B, N, S, rows_per_wg, mask, mask_is_count, inv_n, inv_n_host, ctx_part, S_ctx, W1, ldw1, b1, W2, b2, W3, b3, d_out, x_part, S_x);
    if (!common_ok(C) || rows_per_wg != TM || d_out != HS || x_part || !ctx_part || !h1y || !h2y || !dctx_part || !wpart_y || !x1 || !W1x || !W2x || !W3x
        || !h1x || !h2x || !gpool || !wpart_x || (gx && d_in != HS) || ld_part < HS * ldw1 + HS + 2 * (HS * HS + HS))
        return 1;
    const Bwd2 Q = {x1, {W1x, HS, b1x, W2x, b2x, W3x, b3x}, h1x, h2x, gpool, gp_S, gp_W, gp_ldw, gx_prev, wpart_x, h1y, h2y, gx, dctx_part, wpart_y, ld_part};
    return launch_by_d_in(mlp2_bwd_kernel<true>, mlp2_bwd_kernel<false>, C, stream, Q);
}

int nddm_deepset_reduce(const float *part, int G, int P, int P_main, int G_tail, float *out, void *stream)
{
    if (G <= 0 || P <= 0 || P_main < 0 || P_main > P || G_tail < 0 || G_tail > G) return 1;
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((P + 63) / 64), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), part, G, P, P_main,
                       G_tail, out);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

/* ---- inference: the whole summary network, a trial count per set.
 * Bytes of the work buffer of nddm_deepset_summary: the per-tile pooled partial sums [blocks + 1, B, S, 64] of the pooling MLPs
 * (S = ceil(N / 64)) and, with two blocks or more, the rows [B * N, 64] one equivariant MLP hands to the next (two such buffers,
 * written in turn, from three blocks on).  -1: bad arguments. */
static int summary_y_buffers(int blocks) { return blocks < 2 ? 0 : (blocks == 2 ? 1 : 2); }
long long nddm_deepset_summary_work_bytes(int B, int N, int blocks)
{
    if (B <= 0 || N <= 0 || blocks < 0) return -1;
    const long long S = (N + TM - 1) / TM;
    return 4LL * HS * ((blocks + 1LL) * B * S + summary_y_buffers(blocks) * (long long)B * N);
}

/* x [B, N, d_in] (1 <= d_in <= 4) -> out [B, summary_dim + n_direct]: the summary of the first counts[b] trials of every set b
 * (counts: int32 [B] on the device, clamped to [0, N] for addressing; a set of count 0 gets a non-finite row; NULL: N of every set),
 * then the direct conditions' columns direct[b * direct_stride + .] (NULL: none).  params: 6 (2 blocks + 2) device pointers, host
 * array, in InvariantNetwork.fused_params() order -- W1, b1, W2, b2, W3, b3 of every block's invariant then equivariant MLP, of the
 * pre-pooling and of the post-pooling MLP (hidden width 64; W3 / b3 of the last: summary_dim rows).  work: 16-byte aligned, at least
 * nddm_deepset_summary_work_bytes(B, N, blocks).  blocks + 2 launches on `stream`; no synchronisation, no atomics, no allocation;
 * rows at or beyond a set's count are never read, and nothing but out and work is written.  0, 1: bad arguments, 2: a launch failed. */
int nddm_deepset_summary(const float *x, int d_in, int B, int N, const int *counts, int blocks, const float *const *params, int summary_dim,
                         const float *direct, int n_direct, int direct_stride, float *out, void *work, long long work_bytes, void *stream)
{
    const long long need = nddm_deepset_summary_work_bytes(B, N, blocks);
    if (!direct) n_direct = 0;
    if (need < 0 || !x || d_in < 1 || d_in > DS_MAX || !params || summary_dim < 1 || n_direct < 0 || summary_dim + n_direct > HS || !out || !work
        || (reinterpret_cast<uintptr_t>(work) & 15) || work_bytes < need || (long long)B * ((N + TM - 1) / TM) > 0x7fffffffLL)
        return 1;
    for (int k = 0; k < 6 * (2 * blocks + 2); ++k) if (!params[k]) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int S = (N + TM - 1) / TM, Sp = (B + TM - 1) / TM;
    const long long pool_sz = (long long)B * S * HS, y_sz = (long long)B * N * HS;
    float *pools = static_cast<float *>(work), *ys = pools + (blocks + 1) * pool_sz;
    auto mlp = [&](int k, int ldw1) { const float *const *p = params + 6 * k; return Mlp{p[0], ldw1, p[1], p[2], p[3], p[4], p[5]}; };
    const SetCounts K = {counts, N};
    // the first pooling MLP (block 0's invariant half, or without blocks the pre-pooling MLP) on the raw trials
    const Common C0 = {x, d_in, B, N, S, TM, nullptr, 0, nullptr, 0.0f, nullptr, 0, mlp(0, d_in), HS, nullptr, 0};
    const FwdOut O0 = {nullptr, nullptr, nullptr, pools, HS, nullptr, 0, 0};
    hipLaunchKernelGGL(summary_first_kernel, dim3(B * S), dim3(NT), 0, st, C0, O0, K);
    // every block's equivariant MLP with the pooling MLP that consumes its rows (the next block's invariant half, or the pre-pooling MLP)
    const float *cur = x;
    int d = d_in;
    for (int i = 0; i < blocks; ++i) {
        float *y = i + 1 < blocks ? ys + (i & 1) * y_sz : nullptr;
        const Common C = {cur, d, B, N, S, TM, nullptr, 0, nullptr, 0.0f, pools + i * pool_sz, S, mlp(2 * i + 1, d + HS), HS, nullptr, 0};
        const FwdOut O = {nullptr, nullptr, y, nullptr, HS, nullptr, 0, 0}, O2 = {nullptr, nullptr, nullptr, pools + (i + 1) * pool_sz, HS, nullptr, 0, 0};
        const Mlp P2 = mlp(2 * i + 2, HS);
        if (d == HS) hipLaunchKernelGGL(summary_pair_kernel<true>, dim3(B * S), dim3(NT), 0, st, C, O, P2, O2, K);
        else hipLaunchKernelGGL(summary_pair_kernel<false>, dim3(B * S), dim3(NT), 0, st, C, O, P2, O2, K);
        cur = y;
        d = HS;
    }
    // the MLP after the pooling: B rows, each the mean of its set's partial sums by its set's own count
    const Common Cp = {nullptr, HS, 1, B, Sp, TM, nullptr, 0, nullptr, 0.0f, nullptr, 0, mlp(2 * blocks + 1, HS), summary_dim, pools + blocks * pool_sz, S};
    const FwdOut Op = {nullptr, nullptr, out, nullptr, summary_dim + n_direct, direct, n_direct, direct_stride};
    hipLaunchKernelGGL(summary_post_kernel, dim3(Sp), dim3(NT), 0, st, Cp, Op, K);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"

#ifdef NDDM_TRAIN_STAMPS
extern "C" int nddm_deepset_read_stamps(unsigned long long *out, int cap)
{
    int n = 0;
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(&n, HIP_SYMBOL(nddm_deepset::g_nstamps), sizeof(int));
    if (n > cap) n = cap;
    if (n > 4096) n = 4096;
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(nddm_deepset::g_stamps), sizeof(unsigned long long) * 2 * n);
    int zero = 0;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(nddm_deepset::g_nstamps), &zero, sizeof(int));
    return n;
}
#endif
