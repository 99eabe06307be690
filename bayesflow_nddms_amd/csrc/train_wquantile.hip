// Exact WEIGHTED quantiles of posterior draws, per (data set, parameter), without the draws or the weights leaving the device: the
// step after csrc/train_importance.hip.  theta [B, S, D] float32 and log_w [B, S] float64 (or integer weights [B, S]) -> for K
// probabilities the two neighbouring order statistics of every column and their interpolation in float64.
//
// The definition is on INTEGER weights, so that every route agrees bit for bit: with m the largest finite log_w of the set,
// W_i = rint(exp(log_w_i - m) 2^36) (0 where log_w_i is not finite), 0 <= W_i <= 2^36.  A row is INSIDE if W_i >= 1 and all its D
// components are finite.  The inside rows of a column sorted by value, ties by row index: x_0 <= ... <= x_(n-1) with weights W_0 ..
// W_(n-1), S_k = W_0 + ... + W_k, c_k = 2 S_k - W_k - W_0 (c_0 = 0, c_(k+1) - c_k = W_k + W_(k+1) > 0), T = c_(n-1).  For p: h = p T,
// k the largest index with c_k <= h; k = n - 1: a = b = x_(n-1), g = 0; else a = x_k, b = x_(k+1), g = (h - c_k) / (W_k + W_(k+1));
// quantile = a + (b - a) g, every float64 operation rounded on its own.  With S <= 16384 every integer is <= 2^52: exact in int64
// and as a double.  Equal weights give csrc/train_quantile.hip's rule bit for bit (the scaling is a power of two).
//
// One workgroup per (set, column).  It sorts 64-bit items (key << 32 | row index; rows not inside and the padding get the largest
// item) in LDS with csrc/train_quantile.h's network, the image padded by 8 items per 64 (the bank arithmetic for 8-byte items is
// in that header).  Then every thread takes a contiguous run of sorted items, sums their weights (recomputed from log_w[row]
// by the one inlined function that also formed the mask and w_out -- the same instructions, the same bits -- or gathered from the
// integer weights passed in), the threads scan their runs' integer totals through LDS, and each thread whose run holds the k of a target walks it once more
// and answers.  Integer adds only: any scan order gives the same bits.  No floating-point atomics, nothing grid-wide; a set's
// numbers depend on neither B nor its neighbours.  theta, log_w and the weights passed in are only read.
#include "train_quantile.h"
#include "train_weight.h"

namespace nddm_train {

constexpr int WQ_MAX_PROBS = 16, WQ_MAX_D = 8, WQ_MAX_LOG = 14;   // 16384 draws: 144 KB of padded 8-byte items, one workgroup per CU

struct WQuantArgs {
    int S, D, K;
    const float *theta;
    const double *log_w;
    const long long *w_in;
    double *quant;
    float *order;
    long long *n_positive, *w_out;
    double p[WQ_MAX_PROBS];
};

// (the quantisation, wq_weight: csrc/train_weight.h -- one function, inlined wherever a weight is needed)

template <int LOGN, int T> __global__ __launch_bounds__(T) void weighted_quantiles_kernel(WQuantArgs A)
{
#pragma clang fp contract(off)                                // (h = p T and g = (h - c_k) / (W_k + W_(k+1)): each rounded on its own)
    constexpr int N = 1 << LOGN, R = N / T;                   // R: the run of sorted items a thread owns
    typedef unsigned long long item_t;
    __shared__ __attribute__((aligned(64))) item_t items[N + (N >> 3)];
    __shared__ long long scan[T];
    __shared__ long long w_first, w_last;
    __shared__ int n_s;
    const int t = threadIdx.x, S = A.S, D = A.D, K = A.K;
    const int b = blockIdx.x / D, d = blockIdx.x - b * D;
    const float *th = A.theta + (long long)b * S * D;
    const double *lw = A.log_w ? A.log_w + (long long)b * S : nullptr;
    const long long *wi = A.w_in ? A.w_in + (long long)b * S : nullptr;
    // m: the largest finite log_w (a max: exact in any order)
    double m = 0.0;
    if (lw) {
        double mine = -INFINITY;
        for (int i = t; i < S; i += T) {
            const double v = lw[i];
            if (isfinite(v)) mine = fmax(mine, v);
        }
        scan[t] = __double_as_longlong(mine);
        __syncthreads();
        for (int off = T >> 1; off > 0; off >>= 1) {
            if (t < off) scan[t] = __double_as_longlong(fmax(__longlong_as_double(scan[t]), __longlong_as_double(scan[t + off])));
            __syncthreads();
        }
        m = __longlong_as_double(scan[0]);                   // (-inf: no finite log_w, every weight 0)
        __syncthreads();
    }
    if (t == 0) n_s = 0;
    __syncthreads();
    int cnt = 0;
    for (int i = t; i < N; i += T) {
        item_t item = ~(item_t)0;
        if (i < S) {
            const long long W = lw ? wq_weight(lw[i], m) : wi[i];
            if (d == 0 && A.w_out) A.w_out[(long long)b * S + i] = W;
            const float *row = th + (long long)i * D;
            bool in = W >= 1;
            float mine = 0.0f;
            for (int c = 0; c < D; ++c) {
                const float v = row[c];
                in = in && isfinite(v);
                if (c == d) mine = v;
            }
            if (in) { item = ((item_t)q_key(mine) << 32) | (unsigned)i; ++cnt; }
        }
        items[q_phys(i)] = item;
    }
    if (cnt) atomicAdd(&n_s, cnt);                            // (an integer count: the order does not matter)
    __syncthreads();
    q_sort<item_t, LOGN, T>(items, t);
    const int n = n_s, i0 = t * R;
    // the weight of the sorted item k < n (such an item holds a row index < S)
    auto weight_at = [&](int k) -> long long {
        const unsigned r = (unsigned)items[q_phys(k)];
        return lw ? wq_weight(lw[r], m) : wi[r];
    };
    // first walk of the run: its total; w0 its first weight, wR the next run's first (c_(k+1) of the run's last item needs it)
    long long total = 0, w0 = 0, wR = 0;
#pragma unroll 4
    for (int e = 0; e < R; ++e)
        if (i0 + e < n) {
            const long long W = weight_at(i0 + e);
            if (e == 0) w0 = W;
            if (i0 + e == n - 1) w_last = W;                  // (one thread)
            total += W;
        }
    if (i0 + R < n) wR = weight_at(i0 + R);
    if (t == 0) w_first = w0;
    scan[t] = total;
    __syncthreads();
    for (int off = 1; off < T; off <<= 1) {                  // inclusive scan of the runs' totals (integers: exact)
        const long long v = t >= off ? scan[t - off] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    if (n == 0) {
        if (t < K) {
            const long long o = ((long long)b * K + t) * D;
            A.quant[o + d] = __longlong_as_double(0x7ff8000000000000LL);
            if (A.order) {
                A.order[2 * o + d] = __uint_as_float(0x7fc00000u);
                A.order[2 * o + D + d] = __uint_as_float(0x7fc00000u);
            }
        }
    } else if (i0 < n) {
        const long long W0 = w_first, before = scan[t] - total;
        const double Tt = (double)(2 * scan[T - 1] - w_last - W0);
        // c of the run's first item and of the next run's first (the run that holds n - 1 is open above): c_k is increasing in k, so
        // exactly one run takes a target, and few runs take any -- only those walk a second time
        const long long c_lo = 2 * (before + w0) - w0 - W0, c_hi = 2 * (before + total + wR) - wR - W0;
        const bool open = n - 1 < i0 + R;
        for (int j = 0; j < K; ++j) {
            const double h = A.p[j] * Tt;
            if (!((double)c_lo <= h && (open || h < (double)c_hi))) continue;
            long long Sk = before, wc = w0;
#pragma unroll 4
            for (int e = 0; e < R; ++e) {
                const int k = i0 + e;
                if (k < n) {
                    const bool lastk = k == n - 1;
                    const long long wn = lastk ? 0 : (e + 1 < R ? weight_at(k + 1) : wR);
                    Sk += wc;
                    const long long c = 2 * Sk - wc - W0, step = wc + wn;
                    if ((double)c <= h && (lastk || h < (double)(c + step))) {
                        const float a = q_unkey((unsigned)(items[q_phys(k)] >> 32));
                        const float bb = lastk ? a : q_unkey((unsigned)(items[q_phys(k + 1)] >> 32));
                        const double g = lastk ? 0.0 : (h - (double)c) / (double)step;
                        const long long o = ((long long)b * K + j) * D;
                        A.quant[o + d] = q_lerp((double)a, (double)bb, g);
                        if (A.order) {
                            A.order[2 * o + d] = a;
                            A.order[2 * o + D + d] = bb;
                        }
                    }
                    wc = wn;
                }
            }
        }
    }
    if (t == 0 && d == 0 && A.n_positive) A.n_positive[b] = n;
}

}  // namespace nddm_train

using namespace nddm_train;

extern "C" {

/* Largest S nddm_train_weighted_quantiles takes: what one workgroup's LDS holds of 8-byte items. */
int nddm_train_weighted_quantiles_max_draws(void) { return 1 << WQ_MAX_LOG; }

/* theta [B, S, D] float32 (device, only read).  EXACTLY ONE of log_w [B, S] doubles (device: the log weights, quantised per set as
 * W = rint(exp(log_w - max finite log_w) 2^36), 0 where not finite) and w_in [B, S] 64-bit integers (device: the integer weights
 * themselves, each in [0, 2^36] -- not checked).  probs [K] doubles in HOST memory (copied into the kernel's arguments), 1 <= K <=
 * 16, every p in [0, 1].  quant [B, K, D] doubles; order [B, K, 2, D] float32 (may be null): the two order statistics each quantile
 * lies between; n_positive [B] 64-bit integers (may be null): the rows with W >= 1 and every component finite; w_out [B, S] 64-bit
 * integers (may be null): the quantised weights, written by each set's column-0 workgroup.  1 <= S <= 16384, 1 <= D <= 8.  One
 * launch on `stream`, nothing synchronises, nothing is allocated.
 * -> 0; 1 for a refused shape or a missing argument, before anything is read on the device or launched; 2 for a launch error. */
int nddm_train_weighted_quantiles(int B, int S, int D, const float *theta, const double *log_w, const long long *w_in, const double *probs,
                                  int K, double *quant, float *order, long long *n_positive, long long *w_out, void *stream)
{
    if (B <= 0 || S <= 0 || S > (1 << WQ_MAX_LOG) || D < 1 || D > WQ_MAX_D || K < 1 || K > WQ_MAX_PROBS || !probs) return 1;
    if (!theta || !quant || (log_w == nullptr) == (w_in == nullptr) || (long long)B * D > 0x7fffffffLL) return 1;
    WQuantArgs A = {S, D, K, theta, log_w, w_in, quant, order, n_positive, w_out, {}};
    for (int k = 0; k < K; ++k) {
        if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) return 1;
        A.p[k] = probs[k];
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((long long)B * D));
    if (S <= (1 << 9)) hipLaunchKernelGGL((weighted_quantiles_kernel<9, 64>), grid, dim3(64), 0, st, A);
    else if (S <= (1 << 12)) hipLaunchKernelGGL((weighted_quantiles_kernel<12, 128>), grid, dim3(128), 0, st, A);
    // (1024 threads where the unweighted kernel takes 512 at 2^14: one workgroup fits a CU here, and with 4 waves per SIMD instead of 2
    // the kernel measured 1.43 against 1.74 ms at 500 x 10 000 x 5)
    else hipLaunchKernelGGL((weighted_quantiles_kernel<14, 1024>), grid, dim3(1024), 0, st, A);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
