// Exact order statistics of posterior draws, per (data set, parameter), without the draws leaving the device: the step after
// csrc/train_sample.hip.  theta [B, S, D] float32 -> for K probabilities the two neighbouring order statistics of every column and
// their linear interpolation in float64 (np.quantile's default rule), over the rows INSIDE (every component finite and, with a
// box, within it: train_sample.hip's mask, per ROW).
//
// One workgroup per (set, column).  It reads the set's rows whole (its D - 1 siblings find them in L2), forms the row mask, maps its
// own column to order-preserving 32-bit keys (outside rows and the padding up to the next instantiated power of two get the
// largest key, so they sort to the end and the count of inside rows says where they begin) and sorts the keys in LDS with a
// bitonic network.  The network is walked three strides at a time: a thread holds the 8 keys that differ in three index bits,
// so the 105 compare-exchange stages of 16384 keys are 38 LDS round trips; each phase ends on 8 contiguous keys per thread
// (16-byte accesses).  The LDS image is padded by 8 words per 64: the passes whose lowest stride is 8, 16 or 32 would otherwise
// put a half-wave's 32 lanes on 8, 16 or 32 words of one bank row.  No floating-point atomics: the result is a pure function of
// the set's own rows.  theta is only read.
#include "train_quantile.h"                                   // the key map, the padded image and the network, shared with train_wquantile.hip

namespace nddm_train {

constexpr int Q_MAX_PROBS = 16, Q_MAX_D = 8, Q_MAX_LOG = 15;      // 32768 draws: 144 KB of padded keys, one workgroup per CU

struct QuantArgs {
    int S, D, K;
    const float *theta, *lo, *hi;
    double *quant;
    float *order;
    long long *n_inside;
    double p[Q_MAX_PROBS];
};

template <int LOGN, int T> __global__ __launch_bounds__(T) void draw_quantiles_kernel(QuantArgs A)
{
    constexpr int N = 1 << LOGN;
    __shared__ __attribute__((aligned(32))) unsigned keys[N + (N >> 3)];
    __shared__ int n_s;
    const int t = threadIdx.x, S = A.S, D = A.D, K = A.K;
    const int b = blockIdx.x / D, d = blockIdx.x - b * D;
    const float *th = A.theta + (long long)b * S * D;
    if (t == 0) n_s = 0;
    __syncthreads();
    int cnt = 0;
    for (int i = t; i < N; i += T) {
        unsigned key = 0xFFFFFFFFu;
        if (i < S) {
            const float *row = th + (long long)i * D;
            bool in = true;
            float mine = 0.0f;
            for (int c = 0; c < D; ++c) {
                const float v = row[c];
                in = in && isfinite(v) && (A.lo == nullptr || (v >= A.lo[c] && v <= A.hi[c]));
                if (c == d) mine = v;
            }
            if (in) { key = q_key(mine); ++cnt; }
        }
        keys[q_phys(i)] = key;
    }
    if (cnt) atomicAdd(&n_s, cnt);                            // (an integer count: the order does not matter)
    __syncthreads();
    q_sort<unsigned, LOGN, T>(keys, t);
    const int n = n_s;
    if (t < K) {
        double q = __longlong_as_double(0x7ff8000000000000LL);
        float lo_v = __uint_as_float(0x7fc00000u), hi_v = lo_v;
        if (n > 0) {
            int j;
            const double g = q_position(n, A.p[t], j);
            const int j1 = min(j + 1, n - 1);
            lo_v = q_unkey(keys[q_phys(j)]);
            hi_v = q_unkey(keys[q_phys(j1)]);
            q = q_lerp((double)lo_v, (double)hi_v, g);
        }
        const long long o = ((long long)b * K + t) * D;
        A.quant[o + d] = q;
        if (A.order) {
            A.order[2 * o + d] = lo_v;
            A.order[2 * o + D + d] = hi_v;
        }
    }
    if (t == 0 && d == 0 && A.n_inside) A.n_inside[b] = n;
}

}  // namespace nddm_train

using namespace nddm_train;

extern "C" {

/* Largest S nddm_train_draw_quantiles takes: what one workgroup's LDS holds. */
int nddm_train_draw_quantiles_max_draws(void) { return 1 << Q_MAX_LOG; }

/* theta [B, S, D] float32 (device, only read); lo / hi [D] float32 (device) or both null: the box of the inside rows.
 * probs [K] doubles in HOST memory (copied into the kernel's arguments), 1 <= K <= 16, every p in [0, 1].
 * quant [B, K, D] doubles; order [B, K, 2, D] float32 (may be null): the two order statistics each quantile lies between;
 * n_inside [B] 64-bit integers (may be null).  One launch on `stream`, nothing synchronises, nothing is allocated.
 * -> 0; 1 for a refused shape or a missing argument, before anything is read on the device or launched; 2 for a launch error. */
int nddm_train_draw_quantiles(int B, int S, int D, const float *theta, const float *lo, const float *hi, const double *probs, int K,
                              double *quant, float *order, long long *n_inside, void *stream)
{
    if (B <= 0 || S <= 0 || S > (1 << Q_MAX_LOG) || D < 1 || D > Q_MAX_D || K < 1 || K > Q_MAX_PROBS || !probs) return 1;
    if (!theta || !quant || (lo == nullptr) != (hi == nullptr) || (long long)B * D > 0x7fffffffLL) return 1;
    QuantArgs A = {S, D, K, theta, lo, hi, quant, order, n_inside, {}};
    for (int k = 0; k < K; ++k) {
        if (!(probs[k] >= 0.0 && probs[k] <= 1.0)) return 1;
        A.p[k] = probs[k];
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((long long)B * D));
    if (S <= (1 << 9)) hipLaunchKernelGGL((draw_quantiles_kernel<9, 64>), grid, dim3(64), 0, st, A);
    else if (S <= (1 << 12)) hipLaunchKernelGGL((draw_quantiles_kernel<12, 128>), grid, dim3(128), 0, st, A);
    else if (S <= (1 << 14)) hipLaunchKernelGGL((draw_quantiles_kernel<14, 512>), grid, dim3(512), 0, st, A);
    else hipLaunchKernelGGL((draw_quantiles_kernel<15, 1024>), grid, dim3(1024), 0, st, A);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
