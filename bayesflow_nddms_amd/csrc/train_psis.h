// The arithmetic of Pareto-smoothed importance weights on a SORTED tail (csrc/train_psis.hip's steps after the selection), written so
// that it also compiles for the host: tests/test_flow_psis_cpu.py builds it with a C++ compiler and holds the kernel's own arithmetic
// to the NumPy definition (tests/psis_ref.py).
//
// y_0 <= ... <= y_(n-1), n >= 5: the tail's exceedances exp(x_r) - exp(cutoff) in rank order.  Zhang and Stephens' estimator with the
// PSIS prior:  m_est = 30 + isqrt(n) candidates b_j = (1 - sqrt(m_est / (j - 0.5))) / (3 y_q) + 1 / y_(n-1), q = floor(n / 4 + 0.5) - 1;
// k_j = mean_r log1p(-b_j y_r);  L_j = n (log(-b_j / k_j) - k_j - 1);  w_j = 1 / sum_i exp(L_i - L_j), normalised;  b = sum_j b_j w_j;
// k_raw = mean_r log1p(-b y_r);  sigma = -k_raw / b;  pareto_k = (n k_raw + 5) / (n + 10).  The tail value of rank r becomes
// min(log(q_r + exp(cutoff)), 0) with q_r the fitted distribution's quantile at (r + 0.5) / n.
//
// A mean over the tail is ONE fixed tree over the ranks: lane l of 64 adds the terms r = l, l + 64, ... in that order, then the 64
// partial sums fold by halves (l += l + 32, l += l + 16, ... l += l + 1).  The kernel runs it with a wave per candidate and the host
// with a loop; the result is a function of the sorted values alone.  Every operation is rounded on its own (no contraction).
#pragma once
#include <math.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PSIS_FN __host__ __device__ __forceinline__
#else
#define PSIS_FN inline
#endif

namespace nddm_train {

constexpr int PSIS_LANES = 64;          // the tree's width: a wave
constexpr int PSIS_MAX_TAIL = 384;      // M = min(ceil(S / 5), ceil(3 sqrt(S))) at S = 16384
constexpr int PSIS_MAX_CAND = 64;       // 30 + isqrt(384) = 49 candidates at most
constexpr double PSIS_LOG_DBL_MIN = -708.3964185322641;

PSIS_FN int psis_candidates(int n) { return 30 + (int)sqrt((double)n); }      // (sqrt of a double is correctly rounded: exact at squares)

PSIS_FN int psis_quartile(int n) { return (int)floor((double)n / 4.0 + 0.5) - 1; }

// b_j, j = 1 .. m_est
PSIS_FN double psis_candidate(int j, int m_est, double yq, double ymax)
{
#pragma clang fp contract(off)
    const double r = sqrt((double)m_est / ((double)j - 0.5));
    const double a = (1.0 - r) / (3.0 * yq);
    return a + 1.0 / ymax;
}

// lane's share of sum_r log1p(-b y_r): the terms r = lane, lane + 64, ... in that order
PSIS_FN double psis_lane_partial(double b, const double *y, int n, int lane)
{
#pragma clang fp contract(off)
    double s = 0.0;
    for (int r = lane; r < n; r += PSIS_LANES) {
        const double t = -b * y[r];
        s += log1p(t);
    }
    return s;
}

PSIS_FN double psis_profile(int n, double b, double k)
{
#pragma clang fp contract(off)
    const double l = log(-b / k);
    return (double)n * (l - k - 1.0);
}

// 1 / sum_i exp(L_i - L_j), i in order (an overflowing exp is +inf: weight 0)
PSIS_FN double psis_weight(const double *L, int m_est, int j)
{
#pragma clang fp contract(off)
    double s = 0.0;
    for (int i = 0; i < m_est; ++i) s += exp(L[i] - L[j]);
    return 1.0 / s;
}

// b = sum_j b_j (w_j / sum w), j in order
PSIS_FN double psis_combine(const double *bj, const double *w, int m_est)
{
#pragma clang fp contract(off)
    double sw = 0.0;
    for (int j = 0; j < m_est; ++j) sw += w[j];
    double b = 0.0;
    for (int j = 0; j < m_est; ++j) {
        const double t = bj[j] * (w[j] / sw);
        b += t;
    }
    return b;
}

PSIS_FN double psis_shape(int n, double k_raw)
{
#pragma clang fp contract(off)
    const double t = (double)n * k_raw;
    return (t + 5.0) / ((double)n + 10.0);
}

// whether the tail is replaced at all
PSIS_FN bool psis_applies(double k, double sigma) { return isfinite(k) && isfinite(sigma) && sigma > 0.0; }

// the smoothed log weight of rank r relative to the set's largest: min(log(q_r + e_c), 0)
PSIS_FN double psis_smoothed(int r, int n, double k, double sigma, double e_c)
{
#pragma clang fp contract(off)
    const double p = ((double)r + 0.5) / (double)n;
    const double l = log1p(-p);
    double q;
    if (k == 0.0) q = -sigma * l;
    else {
        const double t = -k * l;
        q = sigma * expm1(t) / k;
    }
    const double s = log(q + e_c);
    return s < 0.0 ? s : 0.0;
}

// ---- the host's walk of the same tree and of the whole fit (the kernel's own walk is in csrc/train_psis.hip)
inline double psis_mean_log1p_host(double b, const double *y, int n)
{
    double v[PSIS_LANES];
    for (int l = 0; l < PSIS_LANES; ++l) v[l] = psis_lane_partial(b, y, n, l);
    for (int off = PSIS_LANES >> 1; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) v[l] = v[l] + v[l + off];
    return v[0] / (double)n;
}

// y [n] sorted, 5 <= n <= PSIS_MAX_TAIL -> pareto_k, sigma; smoothed [n] (may be null): the values of psis_smoothed where the fit applies
inline void psis_fit_host(int n, const double *y, double e_c, double *pareto_k, double *sigma, double *smoothed)
{
    double bj[PSIS_MAX_CAND], Lj[PSIS_MAX_CAND], wj[PSIS_MAX_CAND];
    const int m_est = psis_candidates(n);
    const double yq = y[psis_quartile(n)], ymax = y[n - 1];
    for (int j = 1; j <= m_est; ++j) {
        bj[j - 1] = psis_candidate(j, m_est, yq, ymax);
        Lj[j - 1] = psis_profile(n, bj[j - 1], psis_mean_log1p_host(bj[j - 1], y, n));
    }
    for (int j = 0; j < m_est; ++j) wj[j] = psis_weight(Lj, m_est, j);
    const double b = psis_combine(bj, wj, m_est);
    const double k_raw = psis_mean_log1p_host(b, y, n);
    *sigma = -k_raw / b;
    *pareto_k = psis_shape(n, k_raw);
    if (smoothed && psis_applies(*pareto_k, *sigma))
        for (int r = 0; r < n; ++r) smoothed[r] = psis_smoothed(r, n, *pareto_k, *sigma, e_c);
}

}  // namespace nddm_train
