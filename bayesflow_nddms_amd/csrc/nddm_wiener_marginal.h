// nddm_wiener_marginal.h -- marginal log-likelihood of the single-trial model (NDDM_SINGLE_TRIAL, single_trial_alpha_not_scaled.py:107-155):
// the per-trial boundary a ~ N(mu_alpha, std_alpha^2) | a > 0 is latent, the external datum z1 ~ N(gamma a, sigma1^2) observes it, and the
// response is the first passage of the eta = 0 Wiener process with a' = a / dc, v' = drift / dc, w = beta.  No closed form, but ONE
// one-dimensional integral per (parameter row, trial).  Included by nddm_kernels.hip (one translation unit) after nddm_wiener.h, whose
// wiener_row / wiener_logpdf / wiener_log_survival evaluate the integrand: nothing of them is repeated here.  DESIGN.md section 15.
//
// The quantity.  N(z; gamma a, sigma1^2) N(a; mu, sd^2) = N(z; gamma mu, s2m) N(a; m, tau^2) with s2m = sigma1^2 + gamma^2 sd^2,
// tau^2 = sd^2 sigma1^2 / s2m, m = (mu sigma1^2 + gamma z sd^2) / s2m, so one trial (y = choicert, z = z1) has
//     log L = log N(z; gamma mu, s2m) - log Phi(mu / sd) + log int_0^inf h(a) N(a; m, tau^2) da
//     h(a) = f_W(|y| - ter on the boundary of y's sign | a / dc, drift / dc, beta)     a response      (wiener_logpdf at eta = 0)
//          = P(T > t_censor | a / dc, drift / dc, beta)                                 y == 0, a timeout (wiener_log_survival, both forms)
// A timeout carries no time in this model's output: t_censor (the decision-time cap, max_steps dt) is an argument of the call.
//
// The rule.  In x = log a (the integrand's cut at small a, e^{-pi^2 t / (2 a'^2)}, is doubly exponential and smooth in x; in a it costs a
// Gauss-Legendre rule its convergence), WMARG_PASSES = 3 passes of WMARG_K = 32 Gauss-Legendre nodes: every pass evaluates the log
// integrand l_k at its nodes and keeps them; the first two then ZOOM -- the next window is the span of the nodes within WMARG_BAND = 20.7
// of the largest l_k, widened by one node on each side (or to the window's own end) -- and the last sums by log-sum-exp around its
// maximum.  The integrand is unimodal in x (h is, the Gaussian is), so the node that is largest brackets the peak with its neighbours,
// every node left out lies below e^-20.7 of it, and a pass shrinks a window much wider than the peak about tenfold: two zooms bring a window
// 10 wide in x onto a peak 0.005 wide (tau / m = 0.005, the narrowest in the tests' boxes).  96 evaluations per trial, the same for every
// lane.
//
// The first window must hold the peak of the PRODUCT, which neither factor's own support does: a narrow Gaussian centred where h is
// e^-500 (z far from what the response time says, or m < 0) is tilted by h's slope and peaks tens of tau away from m.  The window is
// the hull of both supports, each end a point where the product is provably far below its value somewhere inside (t the decision
// time, C = WMARG_CUT = 60, L = WMARG_L = 6.5, m+ = max(m, 0), nu the drift toward the other boundary):
//     upper end, a response:  max(c_hi, m+ + L tau),  c_hi = dc (max(-nu t, 0) + sqrt(2 C t)) / w   (h <= e^-C of its peak beyond c_hi:
//                             its large-a form is e^{-(w a' + nu t)^2 / (2t)}; beyond both modes both factors fall)
//     upper end, a timeout:   max(m+, a_1) + L tau,   a_1 = dc max((v' t + 6 sqrt t) / (1 - beta), (-v' t + 6 sqrt t) / beta)  (S is 1 to
//                             2e-9 above a_1 and never larger: from there the Gaussian alone decides)
//     lower end:              c_lo sqrt(C / (2C + E + D)),  c_lo = dc pi sqrt(t / (2C))  (h = e^-C e^{...} at c_lo, rising as e^{-pi^2 t /
//                             (2 a'^2)}),  E = ((c_lo - m)^2 - min(m, 0)^2) / (2 tau^2) for m <= c_lo and 0 otherwise (what the Gaussian gives
//                             back between the cut and c_lo),  D = c_lo |v'| / dc (what the drift term can);  and, for m <= c_lo, not
//                             below m - L tau (h rises there: the Gaussian's own end is good)
// A cut derived from h alone (the first design) left the peak outside on several percent of adversarial trials, by hundreds of log units.
//
// Special values (the math, none an error): a row with a non-finite parameter, std_alpha <= 0, sigma1 <= 0, dc <= 0, beta outside (0, 1)
// or ter < 0 gives NaN for every trial and its sum, its neighbours unaffected; a response with |y| <= ter gives -inf; y == 0 with
// t_censor > 0 is a censored trial, with t_censor <= 0 (or NaN) NaN; a non-finite z1 or a NaN y gives NaN.  A valid row with a valid trial
// never gives NaN or +inf.
//
// Execution: wiener_grad_kernel's.  A wave owns one row, a workgroup of 4 waves WMARG_ROWS = 4 consecutive ones; broadcast layout (the data
// set staged in LDS one WIENER_TILE at a time) when draws_per_dataset >= WIENER_ROWS, paired otherwise.  Lane j accumulates trials j, j + 64,
// ... of the row in that order in float64 and a butterfly of the 64 partial sums gives the row's sum: the bits are a function of (the row's
// parameters, its data set, n_trials, t_censor) alone.  The 32 node values of a pass live in LDS (32 KB per workgroup, lane-interleaved: no
// bank conflict), not in 32 registers of an unrolled loop.  No scratch memory, no atomics; stores are plain vector stores.
#pragma once
#include <type_traits>

#include "nddm_wiener.h"

namespace nddm {

constexpr int WMARG_K = 32;                     // Gauss-Legendre nodes per pass
constexpr int WMARG_PASSES = 3;                 // two zooms and the sum
constexpr float WMARG_BAND = 20.7f;             // a zoom keeps the nodes within e^-20.7 (1e-9) of the largest
constexpr float WMARG_CUT = 60.0f;              // C: h's own support ends where it is e^-60 of its peak
constexpr float WMARG_L = 6.5f;                 // L: the Gaussian's own support, in tau
constexpr int WMARG_RPW = 1;                    // rows per wave
constexpr int WMARG_ROWS = 4 * WMARG_RPW;       // rows per workgroup (4 waves)

// the positive half of the 32-point Gauss-Legendre rule on (-1, 1), nodes and weights (the rule is symmetric)
__device__ constexpr float WMARG_X[16] = {4.830766569e-02f, 1.444719616e-01f, 2.392873623e-01f, 3.318686023e-01f, 4.213512761e-01f, 5.068999089e-01f,
                                          5.877157572e-01f, 6.630442669e-01f, 7.321821187e-01f, 7.944837960e-01f, 8.493676137e-01f, 8.963211558e-01f,
                                          9.349060759e-01f, 9.647622556e-01f, 9.856115115e-01f, 9.972638618e-01f};
__device__ constexpr float WMARG_W[16] = {9.654008851e-02f, 9.563872008e-02f, 9.384439908e-02f, 9.117387870e-02f, 8.765209300e-02f, 8.331192423e-02f,
                                          7.819389579e-02f, 7.234579411e-02f, 6.582222278e-02f, 5.868409348e-02f, 5.099805926e-02f, 4.283589802e-02f,
                                          3.427386291e-02f, 2.539206531e-02f, 1.627439473e-02f, 7.018610009e-03f};

__device__ __forceinline__ float wmarg_node(int k) { return k < 16 ? -WMARG_X[15 - k] : WMARG_X[k - 16]; }
__device__ __forceinline__ float wmarg_weight(int k) { return WMARG_W[k < 16 ? 15 - k : k - 16]; }

struct WienerMarginalArgs {
    const float *params;        // [R, 8]
    const float *data;          // [D, N, 2] = (choicert, z1)
    float *out_trial;           // [R, N] or NULL
    double *out_sum;            // [R] or NULL
    long long R, S;             // rows, rows per data set
    long long chunks;           // workgroups per data set (broadcast layout)
    int N, P;
    float t_censor;
};

// What the marginal needs of a row beyond WienerRow (a struct of its own: wiener_kernel's registers do not change).  The WienerRow beside
// it is wiener_row<NDDM_BASIC_DDM_DC> of (drift, a = dc, beta, tau = 0, dc): the process at a' = 1, which a node rescales to its own a'.
struct WienerMarginalRow {
    float ter, dc, ldc;         // ldc = log dc
    float vp, beta;             // v' = drift / dc
    float k0, k1;               // m = k0 + k1 z
    float tau, i2t2;            // tau, 1 / (2 tau^2)
    float gm, i2s;              // gamma mu, 1 / (2 s2m)
    float c0;                   // -1/2 log(2 pi s2m) - log Phi(mu / sd) - log tau - 1/2 log(2 pi)
    float valid;                // 1 or NaN
};
constexpr int WMARG_ROW_WORDS = sizeof(WienerMarginalRow) / sizeof(float);

// log Phi(x), from nddm_wiener.h's erfcx fit (relative error 1.2e-7 in Phi): below 0 the tail's own exponent is taken out
__device__ __forceinline__ float wmarg_log_phi(float x)
{
    const float z = fabsf(x) * 0.707106781186547524f;
    const float s = 1.0f / fmaf(0.5f, z, 1.0f);
    const float lt = logf(0.5f * s) + wiener_log_erfcx_poly(s) - z * z;            // log of the tail beyond |x|
    return x < 0.0f ? lt : log1pf(-expf(lt));
}

__device__ __forceinline__ WienerRow wiener_marginal_base(const float *p)
{
    const float pb[5] = {p[0], p[5], p[2], 0.0f, p[5]};
    return wiener_row<NDDM_BASIC_DDM_DC>(pb);
}

__device__ __forceinline__ WienerMarginalRow wiener_marginal_row(const float *p)
{
    const float drift = p[0], mu = p[1], beta = p[2], ter = p[3], sd = p[4], dc = p[5], s1 = p[6], g = p[7];
    bool ok = true;
    for (int j = 0; j < 8; ++j) ok = ok && isfinite(p[j]);
    ok = ok && sd > 0.0f && s1 > 0.0f && dc > 0.0f && beta > 0.0f && beta < 1.0f && ter >= 0.0f;
    WienerMarginalRow r;
    const float v1 = s1 * s1, va = sd * sd, s2m = fmaf(g * g, va, v1), is2m = 1.0f / s2m;
    const float tau2 = va * (v1 * is2m);
    r.ter = ter; r.dc = dc; r.ldc = logf(dc);
    r.vp = drift / dc; r.beta = beta;
    r.k0 = mu * (v1 * is2m);
    r.k1 = g * (va * is2m);
    r.tau = sqrtf(tau2);
    r.i2t2 = 0.5f / tau2;
    r.gm = g * mu;
    r.i2s = 0.5f * is2m;
    r.c0 = -1.83787706640934548f - 0.5f * logf(s2m) - wmarg_log_phi(mu / sd) - 0.5f * logf(tau2);
    r.valid = ok ? 1.0f : __builtin_nanf("");
    return r;
}

// log of h(a) N(a; m, tau^2) a at a = e^x, the Gaussian's constant left out: the a' = 1 row rescaled to a' = e^x / dc (every field of
// WienerRow is a power of a' times a constant of the row, or log a' plus one), then nddm_wiener.h's own per-trial code
__device__ __forceinline__ float wiener_marginal_node(const WienerRow &b, const WienerMarginalRow &r, float x, float t, bool censored, int sd, float m)
{
    const float la = x - r.ldc;
    const float ap = __expf(la), a2 = ap * ap, ia2 = __builtin_amdgcn_rcpf(a2);
    WienerRow c = b;
    c.tau = 0.0f;
    c.tstar = b.tstar * a2;
    c.lq = b.lq * ia2;
    c.mq = b.mq * ia2;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        c.m1[s] = b.m1[s] * a2;
        c.m2[s] = b.m2[s] * a2;
        c.w2[s] = b.w2[s] * a2;
        c.cs[s] = b.cs[s] + la;
        c.cl[s] = b.cl[s] - 2.0f * la;
        c.d0[s] = b.d0[s] * ap;
    }
    c.la = la;
    c.ap = ap;
    c.valid = 1.0f;
    const float lh = censored ? wiener_log_survival(c, t) : wiener_logpdf<NDDM_BASIC_DDM_DC>(c, t, sd);
    const float d = fmaf(ap, r.dc, -m);
    return lh + x - (d * d) * r.i2t2;
}

// One trial: `buf` holds a pass's WMARG_K node values, buf[k * stride] (the kernel: LDS, lane-interleaved; a host caller: an array)
__device__ __forceinline__ float wiener_marginal_trial(const WienerRow &b, const WienerMarginalRow &r, float y, float z, float t_censor, float *buf,
                                                       int stride)
{
    const bool censored = y == 0.0f;
    const int sd = y > 0.0f ? 1 : 0;
    const float t0 = censored ? t_censor : fabsf(y) - r.ter;
    const bool dead = !(t0 > 0.0f);                                     // no decision time: -inf for a response, NaN for a timeout
    const bool zbad = !isfinite(z);
    const float t = dead ? 1.0f : fmaxf(t0, 1.0e-30f), zz = zbad ? 0.0f : z;   // (a dead trial runs the same trips on harmless values)
    const float m = fmaf(r.k1, zz, r.k0);
    // the first window: the hull of both supports (file header)
    const float st = sqrtf(t), vt = r.vp * t;
    const float c_lo = r.dc * st * 0.286788218175523f;                  // pi / sqrt(2 C)
    const float mp = fmaxf(m, 0.0f), ltau = WMARG_L * r.tau;
    float hi;
    if (censored) {
        const float a1 = r.dc * fmaxf(fmaf(6.0f, st, vt) / (1.0f - r.beta), fmaf(6.0f, st, -vt) / r.beta);
        hi = fmaxf(mp, a1) + ltau;
    } else {
        const float w = sd ? 1.0f - r.beta : r.beta, nut = sd ? -vt : vt;
        hi = fmaxf(r.dc * (fmaxf(-nut, 0.0f) + st * 10.9544511501033f) / w, mp + ltau);        // sqrt(2 C)
    }
    const bool below = m <= c_lo;
    const float mn = fminf(m, 0.0f);
    const float E = below ? ((c_lo - m) * (c_lo - m) - mn * mn) * r.i2t2 : 0.0f;
    const float D = st * 0.286788218175523f * fabsf(r.vp);
    float lo = c_lo * sqrtf(WMARG_CUT / (2.0f * WMARG_CUT + E + D));
    if (below) lo = fmaxf(lo, m - ltau);
    float xl = logf(fmaxf(lo, 1.0e-30f)), xh = logf(fminf(hi, 1.0e30f));
    float M = 0.0f, xr = 1.0f, sum = 1.0f;
#pragma nounroll
    for (int pass = 0; pass < WMARG_PASSES; ++pass) {
        const float xc = 0.5f * (xh + xl);
        xr = 0.5f * (xh - xl);
        M = -__builtin_inff();
#pragma nounroll
        for (int k = 0; k < WMARG_K; ++k) {
            const float l = wiener_marginal_node(b, r, fmaf(xr, wmarg_node(k), xc), t, censored, sd, m);
            buf[k * stride] = l;
            M = fmaxf(M, l);
        }
        M = fmaxf(M, -3.0e38f);                                         // (every node at -inf: the sum below is 0 and the result -inf, not NaN)
        if (pass < WMARG_PASSES - 1) {                                  // zoom: the span of the nodes within the band, one node wider
            int first = WMARG_K - 1, last = 0;
            for (int k = 0; k < WMARG_K; ++k) {
                const bool in = buf[k * stride] >= M - WMARG_BAND;
                first = in && k < first ? k : first;
                last = in ? k : last;
            }
            if (first > last) { first = 0; last = WMARG_K - 1; }        // (no node compares: a NaN somewhere; the result is NaN anyway)
            const float nxl = first == 0 ? xl : fmaf(xr, wmarg_node(first - 1), xc);
            const float nxh = last == WMARG_K - 1 ? xh : fmaf(xr, wmarg_node(last + 1), xc);
            xl = nxl; xh = nxh;
        } else {
            sum = 0.0f;
            for (int k = 0; k < WMARG_K; ++k) sum = fmaf(wmarg_weight(k), __expf(buf[k * stride] - M), sum);
        }
    }
    const float dz = zz - r.gm;
    float out = r.c0 - (dz * dz) * r.i2s + M + logf(sum) + logf(xr);
    if (dead) out = censored ? __builtin_nanf("") : -__builtin_inff();
    if (zbad || y != y) out = __builtin_nanf("");
    return out * r.valid * b.valid;
}

// The ragged entry point's arguments (nddm_wiener_marginal_log_likelihood_ragged): WienerMarginalArgs' fields in their places, then its own.
// A struct of its own, so that the two kernels of the plain entry point keep their kernel-argument segment and their code.
struct WienerMarginalRaggedArgs {
    const float *params;        // [R, cols]
    const float *data;          // [D, N, 2] = (choicert, z1); set d's pairs at and beyond counts[d] are never read
    float *out_trial;           // [R, N] or NULL
    double *out_sum;            // [R] or NULL
    long long R, S;
    long long chunks;
    int N, P;                   // N: the padded length, the stride of data and out_trial; P: the model's 8 (wiener_launch's; unused)
    float t_censor;
    int cols;                   // 7 (gamma = 1) or 8
    const int *counts;          // [D] trials per set or NULL (every set has N)
};

// STAGED: the workgroup's rows all score one data set, read from LDS (broadcast layout); else every row reads its own (paired layout).
// RAGGED: a trial count per data set and rows of 7 or 8 columns (WienerMarginalRaggedArgs): instantiations of their own.  A row sweeps the
// trials below its set's count n in the order a call at n_trials = n would, so its sum has that call's bits; out_trial beyond n is 0.  A
// count outside [1, N] reads no data and gives NaN in the row's sum and its N per-trial values.  Broadcast layout: the workgroup's rows
// share one set, so n is a function of blockIdx alone and the staging barriers stay uniform; paired: no barrier, a count per wave.
template <bool STAGED, bool RAGGED = false>
__global__ __launch_bounds__(256) void wiener_marginal_kernel(typename std::conditional<RAGGED, WienerMarginalRaggedArgs, WienerMarginalArgs>::type G)
{
    __shared__ float2 tile[STAGED ? WIENER_TILE : 1];
    __shared__ float nodes[WMARG_K * 256];                              // a pass's node values, [k][thread]
    static_assert(WMARG_RPW == 1, "a wave holds one row");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WienerWaveRow w = wiener_wave_row<STAGED, WMARG_ROWS>(G.R, G.S, G.chunks, wave);
    if (!STAGED && !w.has_row) return;
    float q[8];                                                         // (RAGGED: the row as 8 columns, registers)
    const float *p;
    int n = G.N;                                                        // the trials the row sweeps
    bool count_ok = true;
    if constexpr (RAGGED) {
        const float *src = G.params + w.row * G.cols;
#pragma unroll
        for (int j = 0; j < 7; ++j) q[j] = src[j];
        q[7] = G.cols == 8 ? src[7] : 1.0f;
        p = q;
        if (G.counts) {
            const int c = G.counts[(STAGED ? w.rbase : w.row) / G.S];   // (STAGED: one scalar load per workgroup, rbase is blockIdx's)
            count_ok = c >= 1 && c <= G.N;
            n = count_ok ? c : 0;
        }
    } else {
        p = G.params + w.row * G.P;
    }
    // every lane works out the row's constants; the wave keeps lane 0's copy as uniform values
    WienerRow b;
    WienerMarginalRow r;
    {
        const WienerRow mine = wiener_marginal_base(p);
        const WienerMarginalRow rmine = wiener_marginal_row(p);
        const float *m = reinterpret_cast<const float *>(&mine), *rm = reinterpret_cast<const float *>(&rmine);
        float *bw = reinterpret_cast<float *>(&b), *rw = reinterpret_cast<float *>(&r);
#pragma unroll
        for (int f = 0; f < WIENER_ROW_WORDS; ++f) bw[f] = wiener_bcast(m[f], 0);
#pragma unroll
        for (int f = 0; f < WMARG_ROW_WORDS; ++f) rw[f] = wiener_bcast(rm[f], 0);
    }
    float *buf = nodes + threadIdx.x;
    double s = 0.0;
    float *dst = G.out_trial ? G.out_trial + w.row * (long long)G.N : nullptr;
    const auto trial = [&](int t, float x0, float x1) {
        const float lf = wiener_marginal_trial(b, r, x0, x1, G.t_censor, buf, 256);
        if (dst) dst[t] = lf;
        s += (double)lf;
    };
    if constexpr (RAGGED) {
        wiener_row_trials<STAGED, false>(tile, G.data, G.S, G.N, n, w, lane, trial);
        if (dst && w.has_row) {                                         // the padding's values: 0, or NaN under an invalid count
            const float fill = count_ok ? 0.0f : __builtin_nanf("");
            for (int t = n + lane; t < G.N; t += 64) dst[t] = fill;
        }
    } else {
        wiener_row_trials<STAGED, false>(tile, G.data, G.S, G.N, w, lane, trial);
    }
    if (!G.out_sum || !w.has_row) return;
    s = wiener_wave_sum(s);
    if (RAGGED && !count_ok) s = __builtin_nan("");
    if (lane == 0) G.out_sum[w.row] = s;
}

}  // namespace nddm
