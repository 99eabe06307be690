// train_importance.hip -- importance weights of the amortizer's draws against the exact posterior, and what follows from them, one
// workgroup per data set (amortizer.py::importance_weights, AmortizedPosterior.posterior_importance):
//     log w = log p(data | theta) + log p(theta) - log q(theta | data)
// with theta [B, S, D] and log q [B, S] the fused sampler's (train_sample.hip), log p(data | theta) [B, S] float64 the Wiener
// likelihood launch's, and log p(theta) evaluated here, in float64, from a table of per-column descriptors the host builds
// (priors.py::prior_table: kind, two shape parameters, low, high, log normaliser).
//
// The weight of a draw, in this order:
//     a component outside [low, high] or not finite         -> log prior -inf: weight 0 whatever the likelihood holds   (n_zero)
//     else log lik or log q NaN                             -> weight 0, counted apart                                   (n_nan)
//     else log lik -inf, or log w = -inf                    -> weight 0                                                  (n_zero)
//     else log w = +inf (log q = -inf, log lik = +inf)      -> weight 0, no number to normalise by                       (n_nan)
// Two sweeps over a set's draws, the SAME loop body (one copy of the code: both sweeps form the same bits of log w):
//     sweep 0: the maximum m of log w (exact: any order), the counts, log w itself if asked for;
//     sweep 1: the float64 sums of u = exp(log w - m), u^2, u theta_d, u theta_d^2 -- each thread its rows t, t + NT, ... in index
//              order, then a fixed halving tree over the threads in LDS: bit-reproducible, no floating-point atomics, and a set's
//              numbers depend on neither B nor its neighbours (nothing is grid-wide).
// Out: log_evidence = m + log(sum u / S) (by S: a draw outside the prior's support is a draw of q whose weight IS zero),
// ess = (sum u)^2 / sum u^2, max_share = 1 / sum u (the draw at the maximum has u = 1), the weighted mean and sd (ddof 0, the
// variance clamped at 0 before the root).  A set without a positive weight: nan mean, sd and max_share, ess 0, log_evidence -inf.
// 28 bytes a draw: at B = 1 this is one workgroup waiting on memory latency, a few microseconds; it is not contorted to hide that.
#include <hip/hip_runtime.h>
#include <math.h>

namespace nddm_train {

constexpr int NT = 256;            // threads per workgroup: four waves, 40 rows each at S = 10 000
constexpr int ID_MAX = 8;          // columns at most
constexpr int NQ = 2 + 2 * ID_MAX; // sums per set
constexpr int PRIOR_LD = 6;        // doubles per column descriptor: kind, p1, p2, low, high, log normaliser
enum { PRIOR_NORMAL = 0, PRIOR_TRUNCNORMAL = 1, PRIOR_BETA = 2, PRIOR_UNIFORM = 3, PRIOR_FIXED = 4 };

struct ImportanceOut { double *log_evidence, *ess, *max_share, *mean, *sd; long long *n_zero, *n_nan; double *log_w; };

// log density of one column (the table's row pr) at x, -inf outside [low, high] or at a non-finite x
__device__ __forceinline__ double log_prior_column(const double *pr, double x)
{
    const double ninf = -INFINITY;
    const int kind = (int)pr[0];
    const double p1 = pr[1], p2 = pr[2], lo = pr[3], hi = pr[4], ln = pr[5];
    if (!isfinite(x) || x < lo || x > hi) return ninf;
    if (kind == PRIOR_NORMAL || kind == PRIOR_TRUNCNORMAL) {      // p1 mean, p2 sd
        const double u = (x - p1) / p2;
        return -0.5 * u * u - ln;
    }
    if (kind == PRIOR_BETA) {                                     // p1 a, p2 b; a term with exponent 0 is 0 (also at the edge)
        const double ta = p1 == 1.0 ? 0.0 : (p1 - 1.0) * log(x), tb = p2 == 1.0 ? 0.0 : (p2 - 1.0) * log1p(-x);
        return ta + tb - ln;
    }
    return -ln;                                                   // uniform: log(high - low); fixed: 0
}

__global__ __launch_bounds__(NT) void importance_kernel(int S, int D, const float *theta, const float *log_q, const double *log_lik,
                                                        const double *prior, ImportanceOut O)
{
    __shared__ double red[NQ][NT];
    __shared__ double pr_s[ID_MAX * PRIOR_LD];
    __shared__ long long cnt[2][NT];
    const int t = threadIdx.x, b = blockIdx.x;
    const long long r0 = (long long)b * S;
    const double ninf = -INFINITY;
    if (t < D * PRIOR_LD) pr_s[t] = prior[t];
    __syncthreads();
    double m = ninf;
    long long nz = 0, nn = 0;
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < 2; ++sweep) {
        for (int s = t; s < S; s += NT) {
            const float *th = theta + (r0 + s) * D;
            double lp = 0.0;
            for (int d = 0; d < D; ++d) lp += log_prior_column(pr_s + d * PRIOR_LD, (double)th[d]);
            const double ll = log_lik[r0 + s], lq = (double)log_q[r0 + s];
            double lw;
            int what = 0;                                         // 0 a weight, 1 zero, 2 a NaN
            if (lp == ninf) { lw = ninf; what = 1; }
            else if (isnan(ll) || isnan(lq)) { lw = ninf; what = 2; }
            else if (ll == ninf) { lw = ninf; what = 1; }
            else {
                lw = ll + lp - lq;
                if (isnan(lw) || lw == INFINITY) { lw = ninf; what = 2; }
                else if (lw == ninf) what = 1;
            }
            if (sweep == 0) {
                m = fmax(m, lw);
                nz += what == 1;
                nn += what == 2;
                if (O.log_w) O.log_w[r0 + s] = lw;
            } else if (what == 0) {
                const double u = exp(lw - m);                     // (m is finite here: this draw's log w is)
                if (u > 0.0) {
                    acc[0] += u;
                    acc[1] += u * u;
#pragma unroll
                    for (int d = 0; d < ID_MAX; ++d)
                        if (d < D) { const double v = (double)th[d]; acc[2 + d] += u * v; acc[2 + ID_MAX + d] += u * (v * v); }
                }
            }
        }
        if (sweep == 0) {                                         // the set's maximum and counts, to every thread
            red[0][t] = m; cnt[0][t] = nz; cnt[1][t] = nn;
            __syncthreads();
            for (int off = NT / 2; off > 0; off >>= 1) {
                if (t < off) { red[0][t] = fmax(red[0][t], red[0][t + off]); cnt[0][t] += cnt[0][t + off]; cnt[1][t] += cnt[1][t + off]; }
                __syncthreads();
            }
            m = red[0][0];
            __syncthreads();
        } else {
#pragma unroll
            for (int q = 0; q < NQ; ++q) red[q][t] = acc[q];
            __syncthreads();
            for (int off = NT / 2; off > 0; off >>= 1) {          // the fixed tree: thread t takes t + off
                if (t < off) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) red[q][t] += red[q][t + off];
                }
                __syncthreads();
            }
        }
    }
    const double sw = red[0][0], sw2 = red[1][0];
    const bool any = sw > 0.0;
    if (t == 0) {
        O.log_evidence[b] = any ? m + log(sw / (double)S) : ninf;
        O.ess[b] = any ? sw * sw / sw2 : 0.0;
        O.max_share[b] = any ? 1.0 / sw : NAN;
        O.n_zero[b] = cnt[0][0];
        O.n_nan[b] = cnt[1][0];
    }
    if (t < D) {
        const double mean = red[2 + t][0] / sw, var = red[2 + ID_MAX + t][0] / sw - mean * mean;
        O.mean[(long long)b * D + t] = any ? mean : NAN;
        O.sd[(long long)b * D + t] = any ? sqrt(fmax(var, 0.0)) : NAN;
    }
}

}  // namespace nddm_train

using namespace nddm_train;

extern "C" {

/* theta [B, S, D] floats (D <= 8), log_q [B, S] floats, log_lik [B, S] doubles, prior [D, 6] doubles (kind 0 normal, 1 truncated normal,
 * 2 beta, 3 uniform, 4 fixed; p1, p2; low, high; the log normaliser) -- all device pointers.  Out, per set: log_evidence, ess, max_share
 * [B] doubles, mean, sd [B, D] doubles, n_zero, n_nan [B] 64-bit integers; log_w [B, S] doubles or NULL.  The rule and the summation
 * order: the head of this file.  Everything on `stream`, nothing synchronises.
 * -> 0; 1 for a shape it refuses or a missing argument, before anything is read or launched; 2 for a launch error. */
int nddm_train_importance(int B, int S, int D, const float *theta, const float *log_q, const double *log_lik, const double *prior,
                          double *log_evidence, double *ess, double *max_share, double *mean, double *sd, long long *n_zero,
                          long long *n_nan, double *log_w, void *stream)
{
    if (B <= 0 || S <= 0 || D < 1 || D > ID_MAX) return 1;
    if (!theta || !log_q || !log_lik || !prior || !log_evidence || !ess || !max_share || !mean || !sd || !n_zero || !n_nan) return 1;
    const ImportanceOut O = {log_evidence, ess, max_share, mean, sd, n_zero, n_nan, log_w};
    hipLaunchKernelGGL(importance_kernel, dim3((unsigned)B), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), S, D, theta, log_q, log_lik,
                       prior, O);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
