// Pareto-smoothed importance weights and the k-hat diagnostic, per data set, without the weights leaving the device: the step after
// csrc/train_importance.hip.  log_w [B, S] float64 -> pareto_k, sigma, cutoff [B] float64, n_tail [B], and (optionally) the smoothed
// log weights [B, S].
//
// The definition, float64 throughout, one set: a log weight that is not finite is a weight of zero; m the largest finite log_w, x_i =
// log_w_i - m (-inf where not finite); M = min(ceil(S / 5), ceil(3 sqrt(S))) comes from the host; c the order statistic of rank S - M - 1
// of x (ascending, 0-based; -inf if that rank is negative), cutoff = max(c, log DBL_MIN); the tail is the rows with x_i > cutoff
// (strictly: n <= M), ordered by value, ties by row index; n <= 4 or no finite log weight: pareto_k = +inf, nothing is replaced.  y_r =
// exp(x_(r)) - exp(cutoff) goes through csrc/train_psis.h's fit; where pareto_k and sigma are finite and sigma > 0 the tail row of rank
// r becomes m + min(log(q_r + exp(cutoff)), 0).  Every other row keeps its input bits.
//
// One workgroup per set.  It sorts the order-preserving 64-bit keys of the x_i in LDS with csrc/train_quantile.h's network (rows that
// are not finite and the padding get key 0, the low end, so rank S - M - 1 of the set is item N - M - 1 of the padded image whatever
// S), reads the cutoff, and reuses the image: every thread counts the tail rows of its own contiguous run of rows, the counts are
// scanned, and the at most M rows land in LDS in row order.  Each tail row counts the rows before it in (value, row) order -- n^2
// comparisons, n <= 384 -- and writes its exceedance at its rank.  The candidates of the fit are spread over the waves, a wave per
// candidate, lanes over the ranks (the header's fixed tree, folded with shuffles).  No floating-point atomics, nothing grid-wide: a
// set's numbers depend on neither B nor its neighbours, and are unchanged by a permutation of distinct rows.  log_w is only read.
#include "train_psis.h"
#include "train_quantile.h"

namespace nddm_train {

constexpr int PS_MAX_LOG = 14;          // 16384 draws: 144 KB of padded 8-byte keys, one workgroup per CU

struct PsisArgs {
    int S, M;
    const double *log_w;
    double *out, *pareto_k, *sigma, *cutoff;
    long long *n_tail;
};

// double -> key with the doubles' order (finite values): csrc/train_quantile.h's q_key on 64 bits.  No finite value maps to 0.
__device__ __forceinline__ unsigned long long ps_key(double v)
{
    unsigned long long u = (unsigned long long)__double_as_longlong(v);
    if ((u << 1) == 0ull) u = 0ull;
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double ps_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}

// the header's tree over a wave: every lane passes its partial sum, every lane gets the total of lane 0's tree
__device__ __forceinline__ double ps_wave_mean(double b, const double *y, int n, int lane)
{
#pragma clang fp contract(off)
    double v = psis_lane_partial(b, y, n, lane);
#pragma unroll
    for (int off = PSIS_LANES >> 1; off > 0; off >>= 1) v = v + __shfl_down(v, off, PSIS_LANES);
    return __shfl(v, 0, PSIS_LANES) / (double)n;
}

// TC: the largest M an instantiation meets (S <= 2^LOGN)
template <int LOGN, int T, int TC> __global__ __launch_bounds__(T) void pareto_smooth_kernel(PsisArgs A)
{
#pragma clang fp contract(off)
    constexpr int N = 1 << LOGN, R = N / T, NW = T / PSIS_LANES;
    typedef unsigned long long item_t;
    struct Tail {                                                 // what the image holds after the selection
        double x[TC], y[TC], bj[PSIS_MAX_CAND], Lj[PSIS_MAX_CAND], wj[PSIS_MAX_CAND];
        int row[TC], ranked_row[TC];
    };
    __shared__ __attribute__((aligned(64))) item_t items[N + (N >> 3)];
    __shared__ long long scan[T];
    static_assert(sizeof(Tail) <= sizeof(item_t) * (N + (N >> 3)), "the tail does not fit the image");
    Tail &tail = *reinterpret_cast<Tail *>(items);
    const int t = threadIdx.x, lane = t & (PSIS_LANES - 1), wave = t / PSIS_LANES, S = A.S, M = A.M, b = blockIdx.x;
    const double *lw = A.log_w + (long long)b * S;
    double *out = A.out ? A.out + (long long)b * S : nullptr;
    // m: the largest finite log_w (a max: exact in any order)
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
    const double m = __longlong_as_double(scan[0]);
    __syncthreads();
    double k = INFINITY, sigma = __longlong_as_double(0x7ff8000000000000LL), cutoff = PSIS_LOG_DBL_MIN, e_c = 0.0;
    int n = 0;
    bool apply = false;
    if (m != -INFINITY) {                                         // (uniform: m is the workgroup's)
        for (int i = t; i < N; i += T) {
            item_t key = 0;
            if (i < S) {
                const double v = lw[i];
                if (isfinite(v)) key = ps_key(v - m);
            }
            items[q_phys(i)] = key;
        }
        __syncthreads();
        q_sort<item_t, LOGN, T>(items, t);
        const item_t ckey = items[q_phys(N - M - 1)];             // (1 <= M <= TC < N: inside the image; a padding item or a zero weight: -inf)
        cutoff = fmax(ckey == 0 ? -INFINITY : ps_unkey(ckey), PSIS_LOG_DBL_MIN);
        __syncthreads();                                          // the image is the tail's from here
        // the tail rows of this thread's run of rows, counted, scanned, written in row order
        const int i0 = t * R;
        int cnt = 0;
        for (int e = 0; e < R; ++e)
            if (i0 + e < S) {
                const double v = lw[i0 + e];
                cnt += isfinite(v) && v - m > cutoff;
            }
        scan[t] = cnt;
        __syncthreads();
        for (int off = 1; off < T; off <<= 1) {
            const long long v = t >= off ? scan[t - off] : 0;
            __syncthreads();
            scan[t] += v;
            __syncthreads();
        }
        n = (int)scan[T - 1];
        n = n < TC ? n : TC;                                      // (n <= M <= TC by the selection; the clamp keeps a wrong M inside LDS)
        int pos = (int)scan[t] - cnt;
        if (cnt)
            for (int e = 0; e < R; ++e)
                if (i0 + e < S) {
                    const double v = lw[i0 + e];
                    if (isfinite(v) && v - m > cutoff) {
                        if (pos < TC) { tail.x[pos] = v - m; tail.row[pos] = i0 + e; }
                        ++pos;
                    }
                }
        __syncthreads();
        if (n > 4) {                                              // (uniform)
            e_c = exp(cutoff);
            for (int i = t; i < n; i += T) {
                const double xi = tail.x[i];
                int rank = 0;
                for (int j = 0; j < n; ++j) {
                    const double xj = tail.x[j];
                    rank += xj < xi || (xj == xi && j < i);       // (row order in LDS: j < i is row_j < row_i)
                }
                tail.y[rank] = exp(xi) - e_c;
                tail.ranked_row[rank] = tail.row[i];
            }
            __syncthreads();
            const int m_est = psis_candidates(n);
            const double yq = tail.y[psis_quartile(n)], ymax = tail.y[n - 1];
            for (int j = wave + 1; j <= m_est; j += NW) {         // (uniform per wave)
                const double bj = psis_candidate(j, m_est, yq, ymax);
                const double kj = ps_wave_mean(bj, tail.y, n, lane);
                if (lane == 0) { tail.bj[j - 1] = bj; tail.Lj[j - 1] = psis_profile(n, bj, kj); }
            }
            __syncthreads();
            if (t < m_est) tail.wj[t] = psis_weight(tail.Lj, m_est, t);
            __syncthreads();
            const double bb = psis_combine(tail.bj, tail.wj, m_est);      // (every thread the same sums in the same order)
            const double k_raw = ps_wave_mean(bb, tail.y, n, lane);
            sigma = -k_raw / bb;
            k = psis_shape(n, k_raw);
            apply = psis_applies(k, sigma);
            if (apply && out)
                for (int r = t; r < n; r += T) out[tail.ranked_row[r]] = m + psis_smoothed(r, n, k, sigma, e_c);
        }
    }
    // every row the fit did not replace keeps its bits (the two loops write disjoint rows)
    if (out)
        for (int i = t; i < S; i += T) {
            const double v = lw[i];
            if (!(apply && isfinite(v) && v - m > cutoff)) out[i] = v;
        }
    if (t == 0) {
        A.pareto_k[b] = k;
        A.sigma[b] = sigma;
        A.cutoff[b] = cutoff;
        A.n_tail[b] = n;
    }
}

}  // namespace nddm_train

using namespace nddm_train;

extern "C" {

/* Largest S nddm_train_pareto_smooth takes: what one workgroup's LDS holds of 8-byte keys. */
int nddm_train_pareto_smooth_max_draws(void) { return 1 << PS_MAX_LOG; }

/* log_w [B, S] doubles (device, only read).  M: the tail's size, min(ceil(S / 5), ceil(3 sqrt(S))) -- computed by the caller so that host
 * and device cannot disagree about it; 1 <= M <= S and, with S <= 16384, M <= 384.  out_log_w [B, S] doubles (may be null: the
 * diagnostic alone; must not overlap log_w): the smoothed log weights, every row outside the replaced tail with its input bits;
 * pareto_k, sigma, cutoff [B] doubles and n_tail [B] 64-bit integers.  One launch on `stream`, nothing synchronises, nothing is
 * allocated.
 * -> 0; 1 for a refused shape or a missing argument, before anything is read on the device or launched; 2 for a launch error. */
int nddm_train_pareto_smooth(int B, int S, int M, const double *log_w, double *out_log_w, double *pareto_k, double *sigma, long long *n_tail,
                             double *cutoff, void *stream)
{
    if (B <= 0 || S <= 0 || S > (1 << PS_MAX_LOG) || M < 1 || M > S) return 1;
    if (!log_w || !pareto_k || !sigma || !n_tail || !cutoff || log_w == out_log_w) return 1;
    PsisArgs A = {S, M, log_w, out_log_w, pareto_k, sigma, cutoff, n_tail};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)B);
    // (the tail's capacity of an instantiation is M at its largest S: 68 at 512, 192 at 4096, 384 at 16384; a larger M is refused)
    if (S <= (1 << 9)) {
        if (M > 68) return 1;
        hipLaunchKernelGGL((pareto_smooth_kernel<9, 64, 68>), grid, dim3(64), 0, st, A);
    } else if (S <= (1 << 12)) {
        if (M > 192) return 1;
        hipLaunchKernelGGL((pareto_smooth_kernel<12, 128, 192>), grid, dim3(128), 0, st, A);
    } else {
        if (M > PSIS_MAX_TAIL) return 1;
        hipLaunchKernelGGL((pareto_smooth_kernel<14, 1024, PSIS_MAX_TAIL>), grid, dim3(1024), 0, st, A);
    }
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
