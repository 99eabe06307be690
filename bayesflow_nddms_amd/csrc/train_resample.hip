// Sampling-importance-resampling of posterior draws, per data set, without the draws or the weights leaving the device: the step after
// csrc/train_importance.hip (and csrc/train_psis.hip).  theta [B, S, D] float32, log_w [B, S] float64 (or integer weights [B, S]) and one
// 64-bit word per set -> M equally weighted draws of the weighted sample: out [B, M, D], the float32 bits of the chosen rows.
//
// The definition is on INTEGER weights, so that every route agrees on every ancestor index: W_i = wq_weight(log_w_i, m) (csrc/
// train_weight.h: rint(exp(log_w_i - m) 2^36), m the largest finite log_w of the set), V_i = W_i if all D components of row i are
// finite, else 0.  Running sums IN ROW ORDER: C_k = V_0 + ... + V_k, T = C_(S-1) <= 2^50.  The offset U = (r T) >> 64 (the high half
// of the 128-bit product of the set's word r, unsigned, and T), 0 <= U < T.  The systematic comb: t_j = floor((j T + U) / M) for j = 0
// .. M - 1, evaluated in 64 bits as j q + q_U + (j rho + rho_U) div M with T = q M + rho and U = q_U M + rho_U (every term < 2^63 for
// M <= 2^20).  The ancestor a_j is the smallest k with C_k > t_j and out[j, :] = theta[a_j, :].  n_unique counts the rows chosen at
// least once, n_positive the rows with V_i >= 1.  T = 0: every output component NaN, every ancestor -1, n_unique 0.
//
// One workgroup per set, the running sums in LDS (128 KB of 8-byte sums at the cap, 16 384 draws: one workgroup per CU, as csrc/
// train_wquantile.hip).  Three phases: the largest finite log_w (a max: exact in any order); the effective weights, read coalesced
// into the image, then every thread sums a contiguous run of R of them, the threads scan their runs' totals through LDS and walk the
// run a second time to leave the inclusive sums; and per output the comb position, a binary search of the image and the row copy.  The
// image is padded by one item per run: a thread's walk strides R items, which unpadded puts a cycle's lanes on two banks.  Integer adds
// only: any scan order gives the same bits.  No floating-point atomics, nothing grid-wide; a set's outputs depend on neither B nor its
// neighbours.  n_unique comes from one flag bit per row (integer atomics in LDS: the order does not matter).  theta, log_w, the
// weights passed in and the words are only read.
#include "train_weight.h"

namespace nddm_train {

constexpr int RS_MAX_D = 8, RS_MAX_LOG = 14, RS_MAX_OUT = 1 << 20;

struct ResampleArgs {
    int S, D, M;
    const float *theta;
    const double *log_w;
    const long long *w_in;
    const unsigned long long *words;
    float *out;
    int *ancestors;
    long long *n_unique, *n_positive, *w_out;
};

template <int LOGN, int T> __global__ __launch_bounds__(T) void resample_kernel(ResampleArgs A)
{
    constexpr int N = 1 << LOGN, R = N / T;
    constexpr int LOGR = R == 4 ? 2 : 4;
    static_assert(R == (1 << LOGR), "a run is 4 or 16 items");
    typedef unsigned long long u64;
    __shared__ __attribute__((aligned(16))) u64 sums[N + T];                             // the image: item i at i + (i >> LOGR)
    __shared__ long long scan[T];
    __shared__ unsigned flags[N / 32];
    __shared__ int n_pos_s, n_uni_s;
    auto phys = [](int i) { return i + (i >> LOGR); };
    const int t = threadIdx.x, S = A.S, D = A.D, M = A.M;
    const long long b = blockIdx.x;
    const float *th = A.theta + b * S * D;
    const double *lw = A.log_w ? A.log_w + b * S : nullptr;
    const long long *wi = A.w_in ? A.w_in + b * S : nullptr;
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
    if (t == 0) { n_pos_s = 0; n_uni_s = 0; }
    for (int i = t; i < N / 32; i += T) flags[i] = 0u;
    __syncthreads();
    // the effective weights, coalesced, into the image (0 beyond S)
    int cnt = 0;
    for (int i = t; i < N; i += T) {
        long long V = 0;
        if (i < S) {
            const long long W = lw ? wq_weight(lw[i], m) : wi[i];
            if (A.w_out) A.w_out[b * S + i] = W;
            const float *row = th + (long long)i * D;
            bool fin = true;
            for (int c = 0; c < D; ++c) fin = fin && isfinite(row[c]);
            V = fin ? W : 0;
            cnt += V >= 1;
        }
        sums[phys(i)] = (u64)V;
    }
    if (cnt) atomicAdd(&n_pos_s, cnt);                        // (an integer count: the order does not matter)
    __syncthreads();
    // the inclusive scan in row order: a run per thread, the runs' totals through LDS, the run again
    const int i0 = t * R;
    u64 total = 0;
#pragma unroll
    for (int e = 0; e < R; ++e) total += sums[phys(i0) + e];                             // (a run is contiguous in the image)
    scan[t] = (long long)total;
    __syncthreads();
    for (int off = 1; off < T; off <<= 1) {
        const long long v = t >= off ? scan[t - off] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    u64 run = (u64)scan[t] - total;
#pragma unroll
    for (int e = 0; e < R; ++e) {
        run += sums[phys(i0) + e];
        sums[phys(i0) + e] = run;
    }
    const u64 Tt = (u64)scan[T - 1];                          // = C_(S-1): the items beyond S are 0
    __syncthreads();
    const long long ob = b * M;
    if (Tt == 0) {
        for (long long e = t; e < (long long)M * D; e += T) A.out[ob * D + e] = __uint_as_float(0x7fc00000u);
        if (A.ancestors)
            for (int j = t; j < M; j += T) A.ancestors[ob + j] = -1;
    } else {
        const u64 U = __umul64hi(A.words[b], Tt), Mu = (u64)M;
        const u64 q = Tt / Mu, rho = Tt - q * Mu, qU = U / Mu, rhoU = U - qU * Mu;
        for (int j = t; j < M; j += T) {
            const u64 tj = (u64)j * q + qU + ((u64)j * rho + rhoU) / Mu;
            int lo = 0, hi = S - 1;                           // t_j < T = C_(S-1): the answer is in [0, S - 1]
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sums[phys(mid)] > tj) hi = mid;
                else lo = mid + 1;
            }
            atomicOr(&flags[lo >> 5], 1u << (lo & 31));
            if (A.ancestors) A.ancestors[ob + j] = lo;
            const float *row = th + (long long)lo * D;
            float *dst = A.out + (ob + j) * D;
            for (int c = 0; c < D; ++c) dst[c] = row[c];
        }
        __syncthreads();
        int uni = 0;
        for (int i = t; i < N / 32; i += T) uni += __popc(flags[i]);
        if (uni) atomicAdd(&n_uni_s, uni);
        __syncthreads();
    }
    if (t == 0) {
        if (A.n_unique) A.n_unique[b] = n_uni_s;
        if (A.n_positive) A.n_positive[b] = n_pos_s;
    }
}

}  // namespace nddm_train

using namespace nddm_train;

extern "C" {

/* Largest S nddm_train_resample takes: what one workgroup's LDS holds of 8-byte running sums. */
int nddm_train_resample_max_draws(void) { return 1 << RS_MAX_LOG; }

/* Largest M nddm_train_resample takes: the comb's 64-bit terms stay below 2^63 up to here. */
int nddm_train_resample_max_out(void) { return RS_MAX_OUT; }

/* theta [B, S, D] float32 (device, only read).  EXACTLY ONE of log_w [B, S] doubles (device: the log weights, quantised per set as
 * W = rint(exp(log_w - max finite log_w) 2^36), 0 where not finite) and w_in [B, S] 64-bit integers (device: the integer weights
 * themselves, each in [0, 2^36] -- not checked).  words [B] 64-bit (device): a set's word, taken as unsigned; uniform words give a
 * uniform offset of the comb.  out [B, M, D] float32: the resampled rows; ancestors [B, M] 32-bit integers (may be null): the row each
 * came from, -1 in a set of total weight 0 (whose out is NaN); n_unique [B] 64-bit integers (may be null): the rows chosen at least
 * once; n_positive [B] 64-bit integers (may be null): the rows with W >= 1 and every component finite; w_out [B, S] 64-bit integers
 * (may be null): the quantised weights, before the row mask.  1 <= S <= 16384, 1 <= D <= 8, 1 <= M <= 2^20.  One launch on `stream`,
 * nothing synchronises, nothing is allocated.
 * -> 0; 1 for a refused shape or a missing argument, before anything is read on the device or launched; 2 for a launch error. */
int nddm_train_resample(int B, int S, int D, int M, const float *theta, const double *log_w, const long long *w_in,
                        const unsigned long long *words, float *out, int *ancestors, long long *n_unique, long long *n_positive,
                        long long *w_out, void *stream)
{
    if (B <= 0 || S <= 0 || S > (1 << RS_MAX_LOG) || D < 1 || D > RS_MAX_D || M < 1 || M > RS_MAX_OUT) return 1;
    if (!theta || !words || !out || (log_w == nullptr) == (w_in == nullptr)) return 1;
    ResampleArgs A = {S, D, M, theta, log_w, w_in, words, out, ancestors, n_unique, n_positive, w_out};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)B);
    if (S <= (1 << 10)) hipLaunchKernelGGL((resample_kernel<10, 256>), grid, dim3(256), 0, st, A);
    else if (S <= (1 << 12)) hipLaunchKernelGGL((resample_kernel<12, 256>), grid, dim3(256), 0, st, A);
    else hipLaunchKernelGGL((resample_kernel<14, 1024>), grid, dim3(1024), 0, st, A);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
