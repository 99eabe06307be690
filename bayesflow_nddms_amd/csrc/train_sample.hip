// train_sample.hip -- the amortizer's posterior sampler: the INVERSE of the conditional flow of train_kernels.hip as one kernel,
// base normals z [B, S, D] and ONE condition row per data set cond [B, C] -> posterior draws theta [B, S, D] (amortizer.py::
// InvertibleNetwork.inverse_per_set; the reference's amortizer.sample(data, n_samples=10000), basic_ddm_dc.py:218-223), and,
// optionally, a data set's posterior moments without its draws ever reaching memory.
//
// The map, layers LAST to FIRST; in a layer (y1 | y2 = the first d1 | the other d2 columns of the row):
//     sub-network 2 on [y2 | cond] -> (o_s | o_t),  s = clamp * tanh(o_s / clamp),  x1 = (y1 - o_t) * exp(-s)
//     sub-network 1 on [x1 | cond] -> (o_s | o_t),                                  x2 = (y2 - o_t) * exp(-s)
//     u[perm[j]] = (x1 | x2)[j]          (the forward is z[j] = actnorm(x)[perm[j]])
//     x = (u - bias) * exp(-scale)       (the inverse ActNorm)
// with a sub-network  in -> h1 = elu(W1 in + b1) -> h2 = elu(W2 h1 + b2) -> W3 h2 + b3  as the forward has it.
//
// Why this is not the training forward run backwards.  The forward was made for 32 rows with a condition row each; here ten
// thousand rows share ONE condition row, and a workgroup's tile of draws never spans two data sets:
//   * the condition's part of layer 1, W1[:, Dh:] cond_b + b1 -- 128 numbers per (data set, half-layer) -- is computed ONCE, by a
//     prologue kernel, into work[B, 2 L, 128]; a draw's own part is the Dh <= 4 columns of its row, a few FMAs on top of it;
//   * a workgroup takes 128 draws (512 threads) through every half-layer, so the 64 KB of W2 a half-layer stages in LDS serve
//     128 rows (at the training kernel's 16 rows, 10 000 draws would read the twelve W2's 625 times each); W2 and the
//     [128 rows][128 units] activation tile (h1, then h2 in its place) are the LDS: 2 x 66 KB of gfx950's 160 KB, one workgroup
//     and two waves per SIMD on a CU;
//   * layer 2 is v_mfma_f32_32x32x2_f32 (exact f32) on LDS operands read 16 bytes at a time: wave w owns the rows
//     [32 (w & 3), + 32) and the units [64 (w >> 2), + 64) as two 32 x 32 tiles that share the A operand -- 128 MFMAs, 48 LDS
//     reads; layer 3 (<= 8 outputs) is v_mfma_f32_16x16x4_f32, 16 rows per wave, and with the affine inverse the epilogue;
//   * the NEXT half-layer's weights are fetched into registers at the top of a half-layer, as the forward does, and the
//     barriers order LDS only.
// Fused statistics: a draw is INSIDE if its D components are finite and, with a box, within [lo, hi]; a tile leaves the float64
// sums of theta and theta^2 over its inside draws and its count of outside draws (rows summed in index order: eight segments
// of sixteen rows, then the eight segment sums), and a second kernel adds a data set's tiles in index order.  No
// floating-point atomics: the sums are bit-reproducible, and a data set's do not depend on B or on its neighbours.
// The flow's own density at the draw (flow_sample_logq_kernel, the same body with LQ = true): the forward's log|det| is the sum of the
// same soft-clamped log-scales s the affine inverse forms, and of the ActNorm log-scales, so
//     log q(theta | cond) = -|z|^2 / 2 - (D / 2) log 2 pi + sum_{half-layers} sum_d s_d + sum_l sum_d scale[l][d]
// costs a row one float32 add per transformed column: the affine phase leaves s where it read the sub-network's output (o3), and
// after the next barrier thread r adds row r's columns in index order to a register -- half-layers in the kernel's order, so the
// value is bit-reproducible and depends on the row only, like the draw.  Two kernels, not a run-time switch: without log_q the
// instructions are the ones they were.
// gfx950 only.  tests/test_gpu_flow_sample.py holds it to a float64 inverse of the same network, tests/test_gpu_flow_importance.py
// the density to the float64 forward.
#include "train_flow.h"

namespace nddm_train {

constexpr int TS = 128;         // draws per workgroup
constexpr int NS = 512;         // threads per workgroup
constexpr int MS = 8;          // outputs of a sub-network at most: 2 * transformed columns, D <= 8 and d1 = D / 2

struct SampleDims { int L, B, S, D, d1, C, tiles; float clamp; };
struct SampleOut { float *theta; const float *lo, *hi; double *part; int *part_n; float *log_q; };    // part [B * tiles, 2 * D_MAX], part_n [B * tiles], log_q [B, S]

// cb[b, hl, u] = b1[u] + sum_c W1[u][Dh + c] cond[b][c] for the half-layer hl = 2 l + (sub-network 2 ? 1 : 0)
__global__ __launch_bounds__(H) void sample_cond_kernel(SampleDims Q, FlowP P, const float *cond, float *cb)
{
    const int hl = blockIdx.x % (2 * Q.L), b = blockIdx.x / (2 * Q.L), u = threadIdx.x;
    const bool second = hl & 1;
    const HalfP &W = second ? P.layer[hl >> 1].b : P.layer[hl >> 1].a;
    const HalfShape G = half_shape(Q.d1, Q.D - Q.d1, Q.C, second);
    const float *w = W.W1 + u * G.DI + G.Dh, *c = cond + (long long)b * Q.C;
    float acc = 0.0f;
    for (int k = 0; k < Q.C; ++k) acc = fmaf(w[k], c[k], acc);
    cb[(long long)blockIdx.x * H + u] = acc + W.b1[u];
}

template <bool LQ> __device__ __forceinline__ void flow_sample_body(const SampleDims &Q, const FlowP &P, const float *z, const float *cb, const SampleOut &O)
{
    // (LDR, the row stride of W2, W3 and the activation tile: 16-byte aligned rows, 16 consecutive rows on 16 distinct 16-byte slots)
    __shared__ __attribute__((aligned(16))) float w2s[H][LDR];         // W2 [unit][k]
    __shared__ __attribute__((aligned(16))) float hr[TS][LDR];         // h1 [row][unit], then h2 in its place
    __shared__ __attribute__((aligned(16))) float w3s[16][LDR];        // W3 [output][unit]; rows >= M zero (the MFMA tile has 16 columns)
    __shared__ float o3[TS][MS + 1];                                   // layer 3's products, [row][output]
    __shared__ float xs[2][TS][D_MAX];                                 // the rows; the other copy receives the permutation
    __shared__ float an_e[L_MAX][D_MAX], an_b[L_MAX][D_MAX];           // exp(-scale), bias of every ActNorm
    __shared__ int inside_s[TS], n_out_s;
    __shared__ double psum[2 * D_MAX][8];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int b = blockIdx.x / Q.tiles, s0 = (blockIdx.x - b * Q.tiles) * TS, nvr = min(TS, Q.S - s0);
    const int D = Q.D, d1 = Q.d1, d2 = D - d1;
    const long long row0 = (long long)b * Q.S + s0;                    // the tile's first row of z / theta
    const float *cb_b = cb + (long long)b * 2 * Q.L * H;
    const int u1 = t & (H - 1), rg = t >> 7;                           // layer 1: unit, group of 32 rows
    const int ub = 64 * (w >> 2) + (lane & 31), rb = 32 * (w & 3);     // layer 2: the lane's unit in the wave's first tile, the wave's first row
    // one thread's share of the next half-layer's weights: W2 and W3 as the forward fetches them, its unit's W1 columns of the row's
    // own part and hoisted condition number, its two units' b2, its column's b3 (thread (row t / Dt, column t % Dt) of the affine phase)
    // (plain local arrays indexed by unrolled constants: registers.  A literal macro: see the training forward's.)
    f32x4 nw2[H * H / 4 / NS];
    float nw3[MS * H / NS], nw1[4], ncb, nb20, nb21, nb3s, nb3t;
#define NDDM_FETCH_SAMPLE(l_, second_) do {                                                                                    \
        const HalfP &Wn = (second_) ? P.layer[l_].b : P.layer[l_].a;                                                         \
        const HalfShape Gn = half_shape(d1, d2, Q.C, (second_));                                                             \
        const f32x4 *src_ = reinterpret_cast<const f32x4 *>(Wn.W2);                                                          \
        _Pragma("unroll") for (int k = 0; k < H * H / 4 / NS; ++k) nw2[k] = src_[t + NS * k];                               \
        /* (every load unconditional, from a clamped address) */                                                             \
        _Pragma("unroll") for (int k = 0; k < MS * H / NS; ++k) {                                                            \
            const int p_ = t + NS * k; const float v_ = Wn.W3[min(p_, Gn.M * H - 1)]; nw3[k] = p_ < Gn.M * H ? v_ : 0.0f; } \
        _Pragma("unroll") for (int c = 0; c < 4; ++c) {                                                                      \
            const float v_ = Wn.W1[u1 * Gn.DI + min(c, Gn.Dh - 1)]; nw1[c] = c < Gn.Dh ? v_ : 0.0f; }                       \
        ncb = cb_b[(2 * (l_) + ((second_) ? 1 : 0)) * H + u1];                                                               \
        nb20 = Wn.b2[ub]; nb21 = Wn.b2[ub + 32];                                                                             \
        nb3s = Wn.b3[t % Gn.Dt]; nb3t = Wn.b3[Gn.Dt + t % Gn.Dt];                                                            \
    } while (0)
    NDDM_FETCH_SAMPLE(Q.L - 1, true);
    for (int p = t; p < 2 * TS * D_MAX; p += NS) (&xs[0][0][0])[p] = 0.0f;       // (columns >= D and rows >= nvr stay zero)
    for (int p = t; p < 8 * LDR; p += NS) (&w3s[8][0])[p] = 0.0f;                // (M <= 8: the rows 8 .. 15 are never written again)
    if (t < L_MAX * D_MAX) {
        const int l = t / D_MAX, d = t - l * D_MAX;
        const bool in = l < Q.L && d < D;
        const float sc = P.layer[in ? l : 0].scale[in ? d : 0], bi = P.layer[in ? l : 0].bias[in ? d : 0];
        an_e[l][d] = in ? expf(-sc) : 0.0f;
        an_b[l][d] = in ? bi : 0.0f;
    }
    if (t == 0) n_out_s = 0;
    __syncthreads();
    for (int p = t; p < nvr * D; p += NS) { const int r = p / D, c = p - r * D; xs[0][r][c] = z[row0 * D + p]; }
    int cur = 0;
    float lq = 0.0f;                                        // LQ: thread r < TS holds row r's sum of s
    for (int k = 0; k < 2 * Q.L; ++k) {
        const int l = Q.L - 1 - (k >> 1);
        const bool second = !(k & 1);                       // sub-network 2 (conditioned on y2, un-transforms y1) runs first
        const HalfShape G = half_shape(d1, d2, Q.C, second);
        const int Dh = G.Dh, Dt = G.Dt, xh0 = G.xh0, xt0 = G.xt0;
        float (*x)[D_MAX] = xs[cur];
        // this half-layer's weights: out of the registers (fetched a half-layer ago) into LDS
        lds_barrier();                                      // (the previous half-layer's readers of w2s, w3s, hr and writers of xs are done)
        if constexpr (LQ) {                                 // the previous half-layer's s (it transformed the columns this one is conditioned on)
            if (k > 0 && t < TS)
                for (int d = 0; d < Dh; ++d) lq += o3[t][d];
        }
#pragma unroll
        for (int q = 0; q < H * H / 4 / NS; ++q) { const int p4 = t + NS * q; *reinterpret_cast<f32x4 *>(&w2s[p4 >> 5][4 * (p4 & 31)]) = nw2[q]; }
#pragma unroll
        for (int q = 0; q < MS * H / NS; ++q) { const int p = t + NS * q; w3s[p >> 7][p & (H - 1)] = nw3[q]; }
        const float w10 = nw1[0], w11 = nw1[1], w12 = nw1[2], w13 = nw1[3], cbv = ncb, b20 = nb20, b21 = nb21, b3s = nb3s, b3t = nb3t;
        if (k + 1 < 2 * Q.L) {                              // ... and the next one's into the registers (two sites: `second` a constant in each)
            if (second) NDDM_FETCH_SAMPLE(l, false); else NDDM_FETCH_SAMPLE(l - 1, true);
        }
        {   // layer 1: the hoisted condition part + the row's own Dh columns; thread = unit u1, rows [32 rg, 32 rg + 32)
            // (a wave reads one row at a time: broadcasts; its 64 units are consecutive words of the tile's row)
#pragma unroll 8
            for (int i = 0; i < 32; ++i) {
                const int r = 32 * rg + i;
                float a = fmaf(w10, x[r][xh0], cbv);
                if (Dh > 1) a = fmaf(w11, x[r][xh0 + 1], a);
                if (Dh > 2) a = fmaf(w12, x[r][xh0 + 2], a);
                if (Dh > 3) a = fmaf(w13, x[r][xh0 + 3], a);
                hr[r][u1] = elu(a);
            }
        }
        lds_barrier();
        f32x16 acc0, acc1;
        {   // layer 2: lane l holds A[row rb + (l & 31)][k] and B[k][unit ub (+ 32)] = W2[unit][k] for the k's [64 (l >> 5), + 64), four
            // at a time (which k's a lane group takes is free: the MFMA sums over both groups)
#pragma unroll
            for (int i = 0; i < 16; ++i) { acc0[i] = 0.0f; acc1[i] = 0.0f; }
            const float4 *ap = reinterpret_cast<const float4 *>(&hr[rb + (lane & 31)][64 * (lane >> 5)]);
            const float4 *bp0 = reinterpret_cast<const float4 *>(&w2s[ub][64 * (lane >> 5)]);
            const float4 *bp1 = reinterpret_cast<const float4 *>(&w2s[ub + 32][64 * (lane >> 5)]);
#pragma unroll
            for (int q4 = 0; q4 < 16; ++q4) {
                const float4 a = ap[q4], b0 = bp0[q4], b1 = bp1[q4];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc1, 0, 0, 0);
            }
        }
        lds_barrier();                                      // every wave has read its h1 rows: h2 takes their place
        // D: unit = tile base + (l & 31), row = 8 (register / 4) + 4 (l >> 5) + register % 4
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = rb + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
            hr[r][ub] = elu(acc0[i] + b20);
            hr[r][ub + 32] = elu(acc1[i] + b21);
        }
        lds_barrier();
        {   // layer 3, [16 rows x H] x [H x 16 outputs] per wave as v_mfma_f32_16x16x4_f32: lane group kk takes the units [32 kb, + 32),
            // kb = kblock(kk), four at a time, ONE accumulator (mfma_k128's two would be another sum order)
            const int n = lane & 15, kk = lane >> 4, kb = kblock(kk);
            const float4 *ap = reinterpret_cast<const float4 *>(&hr[16 * w + n][32 * kb]);
            const float4 *bp = reinterpret_cast<const float4 *>(&w3s[n][32 * kb]);
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int q4 = 0; q4 < 8; ++q4) {
                const float4 a = ap[q4], bq = bp[q4];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bq.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bq.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bq.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bq.w, acc, 0, 0, 0);
            }
            if (n < MS) {                                   // D: output = l & 15, row = 4 (l >> 4) + register
#pragma unroll
                for (int q = 0; q < 4; ++q) o3[16 * w + 4 * kk + q][n] = acc[q];
            }
        }
        lds_barrier();
        if (t < TS * Dt) {                                  // soft clamp + the affine inverse
            const int r = t / Dt, d = t - r * Dt;
            const float os = o3[r][d] + b3s, ot = o3[r][Dt + d] + b3t;
            const float sv = soft_clamp(os, Q.clamp);
            x[r][xt0 + d] = (x[r][xt0 + d] - ot) * expf(-sv);
            if constexpr (LQ) o3[r][d] = sv;                // (only this thread reads o3[r][d]; layer 3 writes it again three barriers on)
        }
        if (!second) {                                      // the layer's two halves are undone: inverse permutation, inverse ActNorm
            lds_barrier();
            float (*xn)[D_MAX] = xs[cur ^ 1];
            for (int p = t; p < TS * D; p += NS) {
                const int r = p / D, j = p - r * D, pj = P.perm[l][j];
                xn[r][pj] = (x[r][j] - an_b[l][pj]) * an_e[l][pj];
            }
            cur ^= 1;
        }
    }
#undef NDDM_FETCH_SAMPLE
    __syncthreads();
    const float (*x)[D_MAX] = xs[cur];
    if (O.theta)
        for (int p = t; p < nvr * D; p += NS) { const int r = p / D, c = p - r * D; O.theta[row0 * D + p] = x[r][c]; }
    if constexpr (LQ) {
        if (t < nvr) {                                       // (the last half-layer is sub-network 1's: d2 columns)
            for (int d = 0; d < d2; ++d) lq += o3[t][d];
            for (int l = Q.L - 1; l >= 0; --l)
                for (int d = 0; d < D; ++d) lq += P.layer[l].scale[d];
            const float *zr = z + (row0 + t) * D;
            float zz = 0.0f;
            for (int d = 0; d < D; ++d) zz = fmaf(zr[d], zr[d], zz);
            O.log_q[row0 + t] = (-0.5f * zz - (float)D * 0.918938533204672742f) + lq;
        }
    }
    if (O.part) {
        if (t < TS) {
            bool in = t < nvr;
            for (int c = 0; c < D; ++c) {
                const float v = x[t][c];
                in = in && isfinite(v) && (O.lo == nullptr || (v >= O.lo[c] && v <= O.hi[c]));
            }
            inside_s[t] = in ? 1 : 0;
            if (t < nvr && !in) atomicAdd(&n_out_s, 1);      // (an integer count: the order does not matter)
        }
        __syncthreads();
        if (t < 16 * D) {                                    // thread (sum q, segment): sixteen rows in index order
            const int q = t >> 3, seg = t & 7, c = q < D ? q : q - D;
            double acc = 0.0;
            for (int i = 0; i < TS / 8; ++i) {
                const int r = (TS / 8) * seg + i;
                const double v = (double)x[r][c];
                if (inside_s[r]) acc += q < D ? v : v * v;
            }
            psum[q][seg] = acc;
        }
        __syncthreads();
        if (t < 2 * D) {
            double acc = psum[t][0];
            for (int seg = 1; seg < 8; ++seg) acc += psum[t][seg];
            O.part[(long long)blockIdx.x * (2 * D_MAX) + t] = acc;
        }
        if (t == 0) O.part_n[blockIdx.x] = n_out_s;
    }
}

__global__ __launch_bounds__(NS) void flow_sample_kernel(SampleDims Q, FlowP P, const float *z, const float *cb, SampleOut O)
{
    flow_sample_body<false>(Q, P, z, cb, O);
}

__global__ __launch_bounds__(NS) void flow_sample_logq_kernel(SampleDims Q, FlowP P, const float *z, const float *cb, SampleOut O)
{
    flow_sample_body<true>(Q, P, z, cb, O);
}

// a data set's tiles, added in index order
__global__ __launch_bounds__(64) void sample_combine_kernel(SampleDims Q, const double *part, const int *part_n, double *sums, long long *n_outside)
{
    const int b = blockIdx.x, t = threadIdx.x;
    const long long t0 = (long long)b * Q.tiles;
    if (t < 2 * Q.D) {
        double acc = 0.0;
        for (int i = 0; i < Q.tiles; ++i) acc += part[(t0 + i) * (2 * D_MAX) + t];
        sums[(long long)b * 2 * Q.D + t] = acc;
    }
    if (t == 32) {
        long long n = 0;
        for (int i = 0; i < Q.tiles; ++i) n += part_n[t0 + i];
        n_outside[b] = n;
    }
}

}  // namespace nddm_train

using namespace nddm_train;

extern "C" {

int nddm_train_flow_supported(int hidden, int L, int D, int d1, int C);       // train_kernels.hip: the gate, unchanged

/* Bytes of scratch a launch of nddm_train_flow_sample needs (0 for sizes it refuses): the hoisted condition parts
 * [B, 2 L_MAX, 128] floats, then the tiles' partial sums [B * tiles, 16] doubles and outside counts [B * tiles] ints. */
long long nddm_train_flow_sample_work_bytes(int B, int S, int D)
{
    if (B <= 0 || S <= 0 || D < 2 || D > D_MAX) return 0;
    const long long tiles = (S + TS - 1) / TS;
    return (long long)B * 2 * L_MAX * H * 4 + (long long)B * tiles * (2 * D_MAX * 8 + 8);
}

/* z [B, S, D] base normals, cond [B, C] one condition row per data set -> theta [B, S, D] (may be NULL: statistics only).
 * lo, hi [D] (both or neither): the box of the statistics.  sums [B, 2 D] doubles (the sums of theta, then of theta^2, over a
 * set's inside draws) and n_outside [B] 64-bit integers: both or neither (draws only).  work: nddm_train_flow_sample_work_bytes
 * (B, S, D) bytes, 8-byte aligned.  params, perm: as nddm_train_flow_fwd.  log_q [B, S] floats or NULL: the flow's log density at
 * each draw (see the head of this file); the draws, sums and counts have the same bits with it and without.  At least one of theta,
 * sums, log_q.  Everything on `stream`, nothing synchronises.
 * -> 0; 1 for a shape the gate refuses or a missing argument, before anything is read or launched; 2 for a launch error. */
int nddm_train_flow_sample_logq(int hidden, int L, int B, int S, int D, int d1, int C, float clamp, const void *const *params, const int *perm,
                                const float *z, const float *cond, float *theta, const float *lo, const float *hi, double *sums,
                                long long *n_outside, float *log_q, void *work, void *stream)
{
    if (!nddm_train_flow_supported(hidden, L, D, d1, C) || B <= 0 || S <= 0) return 1;
    if (!params || !perm || !z || !cond || !work) return 1;
    if ((!theta && !sums && !log_q) || (sums == nullptr) != (n_outside == nullptr) || (lo == nullptr) != (hi == nullptr)) return 1;
    const long long tiles = (S + TS - 1) / TS;
    if ((long long)B * tiles > 0x7fffffffLL || (long long)B * 2 * L > 0x7fffffffLL || !perm_ok(perm, L, D)) return 1;
    FlowP P = {};
    fill(P, L, D, params, perm);
    const SampleDims Q = {L, B, S, D, d1, C, (int)tiles, clamp};
    float *cb = static_cast<float *>(work);
    double *part = reinterpret_cast<double *>(static_cast<char *>(work) + (long long)B * 2 * L_MAX * H * 4);
    int *part_n = reinterpret_cast<int *>(part + (long long)B * tiles * 2 * D_MAX);
    const SampleOut O = {theta, lo, hi, sums ? part : nullptr, sums ? part_n : nullptr, log_q};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(sample_cond_kernel, dim3(B * 2 * L), dim3(H), 0, st, Q, P, cond, cb);
    if (log_q)
        hipLaunchKernelGGL(flow_sample_logq_kernel, dim3((unsigned)(B * tiles)), dim3(NS), 0, st, Q, P, z, static_cast<const float *>(cb), O);
    else
        hipLaunchKernelGGL(flow_sample_kernel, dim3((unsigned)(B * tiles)), dim3(NS), 0, st, Q, P, z, static_cast<const float *>(cb), O);
    if (sums)
        hipLaunchKernelGGL(sample_combine_kernel, dim3(B), dim3(64), 0, st, Q, static_cast<const double *>(part),
                           static_cast<const int *>(part_n), sums, n_outside);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

/* nddm_train_flow_sample_logq without the density: the draws and / or the statistics. */
int nddm_train_flow_sample(int hidden, int L, int B, int S, int D, int d1, int C, float clamp, const void *const *params, const int *perm,
                           const float *z, const float *cond, float *theta, const float *lo, const float *hi, double *sums,
                           long long *n_outside, void *work, void *stream)
{
    return nddm_train_flow_sample_logq(hidden, L, B, S, D, d1, C, clamp, params, perm, z, cond, theta, lo, hi, sums, n_outside, nullptr, work, stream);
}

}  // extern "C"
