// nddm_wiener.h -- batched Wiener first-passage log-likelihood (gfx950): the density the reference's likelihood-based fits
// evaluate, JAGS dwiener(alpha/varsigma, ndt, beta, delta/varsigma) (basic_ddm_dc_pyjags.py:129-133, alpha_not_scaled.py:170-176,
// jagscode/*.jags) and Stan wiener_lpdf behind diffusion_lpdf (basic_ddm_dc_pystan2.py:119-131, stancode/basic_ddm_dc_test.stan),
// one independent value per (parameter row, trial).  Included by nddm_kernels.hip (one translation unit).  DESIGN.md section 11.
//
// Conventions (the reference's): the evidence starts at beta*a and drifts toward the upper boundary; choice 1 / y > 0 is the upper
// boundary.  Diffusion coefficient s: a' = a/s, v' = v/s, eta' = eta/s.  The lower boundary takes (v', w = beta), the upper one the
// same formula with (-v', 1 - beta).  t = rt - tau, u = t / a'^2.  With the drift v ~ N(nu, eta^2) integrated out in closed form
// (Ratcliff 1978; Blurton et al. 2017):
//     log f(t) = log g(u; w) - 2 log a' + (eta'^2 a'^2 w^2 - 2 a' nu' w - nu'^2 t) / (2 (1 + eta'^2 t)) - 1/2 log(1 + eta'^2 t)
// (eta = 0: the ordinary -a'v'w - v'^2 t / 2), g the standard first-passage density (Navarro & Fuss 2009) in one of two forms:
//     small time  g = (2 pi u^3)^-1/2 sum_{k=-2..2} (w + 2k) exp(-(w + 2k)^2 / (2u))                         for u <  WIENER_U_STAR
//     large time  g = pi sum_{k=1..3} k exp(-k^2 pi^2 u / 2) sin(k pi w)                                      for u >= WIENER_U_STAR
// both FIXED-TRIP (5 and 3 terms: relative truncation error <= 2e-10 for u <= 0.40 and <= 1e-10 for u >= 0.35 over w in
// [0.001, 0.999]; tests/test_wiener_host.py) and both in the log domain, the leading exponent taken out:
//     small: log g = -1/2 log(2 pi) - 3/2 log u - w^2 / (2u) + log(w + (w-2) A + (w+2) B + (w-4) A^3 B + (w+4) A B^3),
//            A = exp(-2 (1-w) / u), B = exp(-2 (1+w) / u)   (the k = -+2 exponents are A^3 B and A B^3: two exponentials)
//     large: log g = log pi + log sin(pi w) - pi^2 u / 2 + log(1 + 4c q^3 + 3 (4c^2 - 1) q^8),  c = cos(pi w), q = exp(-pi^2 u / 2)
//            (sin 2x / sin x = 2 cos x, sin 3x / sin x = 4 cos^2 x - 1: one sin / cos per row and boundary, one exponential per trial)
// A per-lane select between the two, no loop: 3 v_exp_f32, 2 v_log_f32 and 1 v_rcp_f32 per trial (+ 1 of each with eta > 0).
//
// Special values (the math, none an error): t <= 0 (an RT at or below tau) gives -inf; a row with a non-finite parameter, a <= 0,
// s <= 0, beta outside (0, 1), tau < 0 or eta < 0 gives NaN for every trial and its sum, its neighbours unaffected.
//   basic_ddm_dc (rt, choice): choice 0 is the Euler-Maruyama simulator's timeout at rt = max_steps dt + tau, RIGHT-CENSORED:
//     log P(T > t) of both boundaries, in one of two forms selected per trial (wiener_log_survival): below u = WIENER_SURV_U the method
//     of images in the position domain (twelve erfcx-scaled terms, the leading exponent taken out: it does not cancel however wide the
//     boundary or strong the drift), at and above it the large-time survival series
//     S(t) = sum_{sides} (pi / a'^2) e^{-a' v w} sum_k k sin(k pi w) e^{-lambda_k t} / lambda_k,  lambda_k = v'^2/2 + k^2 pi^2 / (2 a'^2),
//     terms added until the next is below 2^-24 of the sum, at most 64 (loops: timeouts are rare; t <= 0 gives log 1 = 0).
//   alpha_not_scaled (y, acc): rt = |y|, upper iff y > 0; Nu clipped to +-5 as the generator does (pyhddmjagsutils.py:102-103);
//     y == 0 (the Euler-Maruyama form's timeout) carries no time: NaN.  simulratcliff never writes one.
//
// Execution: a workgroup of 4 waves owns WIENER_ROWS consecutive parameter rows, a wave WIENER_RPW of them (rows w, w+4, ...).  Lane k
// of a wave works out the constants of its k-th row (all rows of the wave at once) and the wave broadcasts them with v_readlane.
// Lane j accumulates trials j, j+64, j+128, ... of a row in that order in float64, and a butterfly of the 64 partial sums gives the
// row's sum: the order is a function of n_trials alone, not of the layout, the grid or the tile, so a row's sum has the same bits
// whichever launch scores it.  Broadcast layout (draws_per_dataset >= WIENER_ROWS): the workgroup's rows all score one data set,
// staged in LDS one WIENER_TILE of trials at a time and read by every row from there; paired layout: each row reads its trials
// from HBM (each is read once anyway).  No scratch memory, no atomics; stores are plain vector stores.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nddm.h"

namespace nddm {

constexpr float WIENER_U_STAR = 0.375f;         // small-time series below, large-time at and above (both exact to < 1e-9 there)
constexpr int WIENER_RPW = 4;                   // rows per wave
constexpr int WIENER_ROWS = 4 * WIENER_RPW;     // rows per workgroup (4 waves)
constexpr int WIENER_TILE = 1024;               // trials staged in LDS at a time (8 KB); a constant, not a knob
constexpr int WIENER_SURV_TERMS = 64;

// The five *Args structs of the family begin alike -- params, data, two outputs (one for the quantile), R, S, chunks, N, P -- and
// wiener_launch (nddm_kernels.hip) fills those fields by name.  They are not derived from one base: that would move the outputs behind
// the common fields in the kernel-argument segment, the prologues would fetch their arguments differently, and the forward kernel's
// broadcast launch measured 0.3 % slower, outside the spread of the layout below (profiles/r15_wiener_refactor_ab.txt).
struct WienerArgs {
    const float *params;        // [R, P]
    const float *data;          // [D, N, 2]
    float *out_trial;           // [R, N] or NULL
    double *out_sum;            // [R] or NULL
    long long R, S;             // rows, rows per data set
    long long chunks;           // workgroups per data set (broadcast layout)
    int N, P;
};

// The constants of one row, one value per field; side 0 = the lower boundary (w = beta, nu = v'), side 1 = the upper one.
// In log2 units where they feed v_exp_f32 / v_log_f32 (base 2), in natural units where they add to the result.
struct WienerRow {
    float tau, tstar;           // tstar = WIENER_U_STAR a'^2 (small-time series for t < tstar)
    float mq;                   // -pi^2 / (2 a'^2) log2(e): q = 2^(mq t)
    float lq;                   // -pi^2 / (2 a'^2): the large-time exponent, natural units
    float hn2, e2;              // v'^2 / 2, eta'^2
    float w[2], m1[2], m2[2];   // w; -2 (1 -+ w) a'^2 log2(e): A = 2^(m1 / t), B = 2^(m2 / t)
    float w2[2];                // w^2 a'^2 / 2: w^2 / (2u) = w2 / t
    float cs[2], cl[2];         // -1/2 log(2 pi) + log a';  log pi + log sin(pi w) - 2 log a'
    float c4[2], c3[2];         // 4 cos(pi w); 3 (4 cos^2(pi w) - 1)
    float d0[2];                // eta'^2 a'^2 w^2 / 2 - a' nu w
    float s1, cpb;              // sin(pi beta), cos(pi beta) (the survival series' recurrence)
    float la;                   // log a'
    float ap, vp;               // a', v' (the survival's small-time form)
    float valid;                // 1 or NaN
};
constexpr int WIENER_ROW_WORDS = sizeof(WienerRow) / sizeof(float);

template <int MODEL>
__device__ __forceinline__ WienerRow wiener_row(const float *p)
{
    float v, a, beta, tau, eta, s;
    if (MODEL == NDDM_BASIC_DDM_DC) { v = p[0]; a = p[1]; beta = p[2]; tau = p[3]; s = p[4]; eta = 0.0f; }
    else { v = p[0]; a = p[1]; beta = p[2]; tau = p[3]; eta = p[4]; s = p[5]; }
    const bool ok = isfinite(v) && isfinite(a) && isfinite(beta) && isfinite(tau) && isfinite(eta) && isfinite(s) && a > 0.0f && s > 0.0f &&
                    beta > 0.0f && beta < 1.0f && tau >= 0.0f && eta >= 0.0f;
    if (MODEL == NDDM_ALPHA_NOT_SCALED && (v < -5.0f || v > 5.0f)) v = v > 0.0f ? 5.0f : -5.0f;      // pyhddmjagsutils.py:102-103
    const float ap = a / s, vp = v / s, ep = eta / s;
    const float a2 = ap * ap, e2 = ep * ep, la = logf(ap);
    const float log2e = 1.44269504088896341f, pi2h = 4.93480220054467931f;     // pi^2 / 2
    WienerRow c;
    c.tau = tau;
    c.tstar = WIENER_U_STAR * a2;
    c.lq = -pi2h / a2;
    c.mq = c.lq * log2e;
    c.hn2 = 0.5f * (vp * vp);
    c.e2 = e2;
    c.la = la;
    c.ap = ap; c.vp = vp;
    const float sb = sinpif(beta), cb = cospif(beta);
    c.s1 = sb; c.cpb = cb;
    const float lsin = logf(sb);
    for (int side = 0; side < 2; ++side) {
        const float w = side ? 1.0f - beta : beta, nu = side ? -vp : vp, cw = side ? -cb : cb;
        c.w[side] = w;
        c.m1[side] = (-2.0f * (1.0f - w)) * a2 * log2e;
        c.m2[side] = (-2.0f * (1.0f + w)) * a2 * log2e;
        c.w2[side] = 0.5f * (w * w) * a2;
        c.cs[side] = -0.918938533204672742f + la;                      // -1/2 log(2 pi) + log a'
        c.cl[side] = 1.14472988584940017f + lsin - 2.0f * la;           // log pi + log sin(pi w) - 2 log a'
        c.c4[side] = 4.0f * cw;
        c.c3[side] = 3.0f * (4.0f * (cw * cw) - 1.0f);
        c.d0[side] = 0.5f * (e2 * a2 * (w * w)) - ap * nu * w;
    }
    c.valid = ok ? 1.0f : __builtin_nanf("");
    return c;
}

// log P(T > t) of the η = 0 process (basic_ddm_dc's censored timeouts), in one of two forms selected per trial by u = t / a'^2:
// the method of images below WIENER_SURV_U, the large-time series at and above it.
//
// Small time, in the position domain: the density of the evidence at x in (0, a), started at x0 = a w, is
// e^{v (x - x0) - v^2 t / 2} sum_n [phi_t(x - x0 - 2na) - phi_t(x + x0 - 2na)], and integrated over (0, a) every image at c gives
//     I(c) = e^{v (c - x0)} P(N(c + v t, t) in (0, a)) = 1/2 e^{v (c - x0)} [erfc(p) - erfc(q)],
// p the distance (in sqrt(2t)) of the drifted centre c + v t OUTSIDE the interval (negative inside) and q > |p| its distance from the far
// end: a difference of two tail values on the SAME side, which does not cancel.  S = sum_n I(x0 + 2na) - I(-x0 + 2na), n = -1, 0, 1 (the
// next images are below e^{-3 / (2u)} = 1e-11 of the leading one at u < 0.06).  Every product is e^{G - p^2} erfcx(p), and the leading
// image's e^{-p0^2} = e^{-sigma} (p0 > 0: the drift has carried the mass past a boundary) is taken out of all of them, so log S =
// -sigma + log(...) keeps its relative accuracy and its range however small S is; with the leading centre inside, sigma = 0.
// The series cannot serve there: below u of about 0.04 its terms must cancel to e^{-w^2 / (2u)} of their size, which float32 does not
// hold (NaN, or a positive log S, on the wide-boundary rows of the prior); from 0.04 up it is exact to float32, and the images in turn
// would need more terms above u of about 0.1.
constexpr float WIENER_SURV_U = 0.06f;          // images below, series at and above (both within the tests' bars on [0.04, 0.1])

// log(erfcx(z) / s), z >= 0: erfcx(z) = s e^{P(s)}, s = 1 / (1 + z / 2), P the degree-9 Chebyshev fit of Numerical Recipes' erfcc
// (relative error <= 1.2e-7 at every z).  No branch and one reciprocal; its exponent joins the term's own, so a product e^{g} erfcx(z) is
// one exponential.  (The library's erfcxf is three branches and, inlined beside the series, cost the basic kernels two waves per SIMD.)
__device__ __forceinline__ float wiener_log_erfcx_poly(float s)
{
    float P = 0.17087277f;
    P = fmaf(P, s, -0.82215223f); P = fmaf(P, s, 1.48851587f); P = fmaf(P, s, -1.13520398f); P = fmaf(P, s, 0.27886807f);
    P = fmaf(P, s, -0.18628806f); P = fmaf(P, s, 0.09678418f); P = fmaf(P, s, 0.37409196f); P = fmaf(P, s, 1.00002368f);
    return fmaf(P, s, -1.26551223f);
}

// 1/2 e^{g} erfcx(z), z >= 0
__device__ __forceinline__ float wiener_half_exp_erfcx(float g, float z)
{
    const float s = __builtin_amdgcn_rcpf(fmaf(0.5f, z, 1.0f));
    return (0.5f * s) * __expf(fminf(g + wiener_log_erfcx_poly(s), 80.0f));
}

// (The four row constants are read behind an empty asm per trial: without it the compiler hoists the row-uniform products of this rare
// branch out of the trial loop into vector registers that stay live through the density's code, and each basic kernel loses a wave per SIMD.)
#if defined(__HIP_DEVICE_COMPILE__)
#define WIENER_PER_TRIAL(a, b, c, d) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d))
#else
#define WIENER_PER_TRIAL(a, b, c, d) ((void)0)
#endif
__device__ __forceinline__ float wiener_log_survival_small(const WienerRow &row, float t)
{
    float ap = row.ap, vp = row.vp, w0 = row.w[0], w1 = row.w[1];
    WIENER_PER_TRIAL(ap, vp, w0, w1);
    t = fmaxf(t, 1.0e-30f);                                             // (S is 1 long before; 1 / sqrt(2t) stays finite)
    float rs = __builtin_amdgcn_rsqf(2.0f * t);
    rs = rs * fmaf(-t * rs, rs, 1.5f);                                  // one Newton step: 1 / sqrt(2t) to the last bit or two
    const float x0 = ap * w0, a2 = 2.0f * ap;
    const float mL = fmaf(t, vp, x0);                                 // the leading image's drifted centre, and its distance beyond a
    const float mU = fmaf(t, vp, -(ap * w1));
    const float p0 = fmaxf(mU, -mL) * rs;
    const float sigma = p0 > 0.0f ? p0 * p0 : 0.0f;
    // image i = 2 (n + 1) + (negative ? 1 : 0), n = -1, 0, 1, at c = x0 + d: G = sigma + v d; dU, dL = its drifted centre's distance beyond a
    // and below 0 in sqrt(2t) (dU + dL = -a / sqrt(2t) < 0: at most one is positive), p the larger and q minus the smaller.  Trip 2i is
    // the p term, trip 2i + 1 the q term: a loop of twelve and not twelve inlined copies, so that it holds one term's registers
    float acc = 0.0f;
#pragma nounroll
    for (int k = 0; k < 12; ++k) {
        const int i = k >> 1;
        const bool neg = i & 1, far = k & 1;
        const float d = (float)((i >> 1) - 1) * a2 - (neg ? 2.0f * x0 : 0.0f);
        const float G = fmaf(vp, d, sigma), dU = (mU + d) * rs, dL = -(mL + d) * rs;
        const float p = fmaxf(dU, dL), z = far ? -fminf(dU, dL) : p;
        const float h = wiener_half_exp_erfcx(fmaf(-z, z, G), fabsf(z));
        const float term = far ? -h : (p >= 0.0f ? h : __expf(fminf(G, 80.0f)) - h);
        acc = neg ? acc - term : acc + term;
    }
    // acc = S e^{sigma}; with the leading centre inside, sigma = 0 and its image's e^{G} is the 1 that S stays near
    return fminf(0.693147180559945309f * __builtin_amdgcn_logf(fmaxf(acc, 1.17549435e-38f)) - sigma, 0.0f);
}

// Large time: the survival series of both boundaries, with e^{-lambda_1 t} and the larger side weight taken out; sin(k pi w) by the
// Chebyshev recurrence (sin(k pi (1 - beta)) = (-1)^(k+1) sin(k pi beta)); terms added until the next is below 2^-24 of the sum.
__device__ __forceinline__ float wiener_log_survival_large(const WienerRow &c, float t)
{
    const float m = fmaxf(c.d0[0], c.d0[1]);
    const float wl = __expf(c.d0[0] - m), wu = __expf(c.d0[1] - m);
    const float kk = -c.lq;                                             // pi^2 / (2 a'^2)
    const float lam1 = c.hn2 + kk;
    float sk_1 = 0.0f, sk = c.s1, sum = 0.0f;
    for (int k = 1; k <= WIENER_SURV_TERMS; ++k) {
        const float fk = (float)k;
        const float lam = c.hn2 + kk * (fk * fk);
        const float sgn = (k & 1) ? 1.0f : -1.0f;
        const float env = fk * __expf(-kk * (fk * fk - 1.0f) * t) * __builtin_amdgcn_rcpf(lam);
        // stop when the next term's bound (|sin| <= 1) is below 2^-24 of the sum: the term itself can vanish (sin(2 pi / 2) = 0 at
        // beta = 1/2) while later ones do not
        if (k > 1 && env * (wl + wu) < 5.9604644775390625e-08f * fabsf(sum)) break;
        sum += env * (wl * sk + wu * sgn * sk);
        const float sn = 2.0f * c.cpb * sk - sk_1;
        sk_1 = sk; sk = sn;
    }
    return -lam1 * t + m + (1.14472988584940017f - 2.0f * c.la) + 0.693147180559945309f * __builtin_amdgcn_logf(sum);
}

__device__ __forceinline__ float wiener_log_survival(const WienerRow &c, float t)
{
    if (!(t > 0.0f)) return t == t ? 0.0f : t;
    return t < (WIENER_SURV_U / WIENER_U_STAR) * c.tstar ? wiener_log_survival_small(c, t) : wiener_log_survival_large(c, t);
}

// log f of one trial on one boundary: a pure function of (row constants, rt, side)
template <int MODEL>
__device__ __forceinline__ float wiener_logpdf(const WienerRow &c, float rt, int sd)
{
    const float t = rt - c.tau;
    const float w = sd ? c.w[1] : c.w[0];
    // small time (2 exponentials: A, B), for u < WIENER_U_STAR
    const float tc = fmaxf(t, 1.17549435e-38f);                        // (a t below the smallest normal float is evaluated there)
    const float it = __builtin_amdgcn_rcpf(tc);
    const float A = __builtin_amdgcn_exp2f((sd ? c.m1[1] : c.m1[0]) * it);
    const float B = __builtin_amdgcn_exp2f((sd ? c.m2[1] : c.m2[0]) * it);
    const float A3B = (A * A) * (A * B), AB3 = (B * B) * (A * B);
    const float ssum = w + (w - 2.0f) * A + (w + 2.0f) * B + (w - 4.0f) * A3B + (w + 4.0f) * AB3;
    // large time (1 exponential: q), for u >= WIENER_U_STAR
    const float q = __builtin_amdgcn_exp2f(c.mq * t);
    const float q2 = q * q, q4 = q2 * q2, q3 = q2 * q, q8 = q4 * q4;
    const float lsum = 1.0f + (sd ? c.c4[1] : c.c4[0]) * q3 + (sd ? c.c3[1] : c.c3[0]) * q8;
    const bool small = t < c.tstar;
    const float ln2 = 0.693147180559945309f;
    const float lx = ln2 * __builtin_amdgcn_logf(small ? ssum : lsum);
    const float lt = ln2 * __builtin_amdgcn_logf(tc);
    const float rest = small ? (sd ? c.cs[1] : c.cs[0]) - 1.5f * lt - (sd ? c.w2[1] : c.w2[0]) * it
                             : (sd ? c.cl[1] : c.cl[0]) + c.lq * t;
    float lf = lx + rest;
    // drift term, eta' integrated out; with eta = 0 the general form reduces to d0 - hn2 t exactly (a division by 1, log of 1), so the
    // row-uniform branch only skips work
    const float d0 = sd ? c.d0[1] : c.d0[0];
    if (MODEL == NDDM_ALPHA_NOT_SCALED && c.e2 > 0.0f) {                // (basic_ddm_dc has no drift variability)
        const float den = 1.0f + c.e2 * t;
        lf += (d0 - c.hn2 * t) * __builtin_amdgcn_rcpf(den) - (0.5f * ln2) * __builtin_amdgcn_logf(den);
    } else {
        lf += d0 - c.hn2 * t;
    }
    lf = t > 0.0f ? lf : -__builtin_inff();
    return lf * c.valid;
}

template <int MODEL>
__device__ __forceinline__ float wiener_trial(const WienerRow &c, float x0, float x1)
{
    if (MODEL == NDDM_BASIC_DDM_DC) {                                   // (rt, choice): 1 upper, -1 lower, 0 censored timeout
        if (x1 == 0.0f) return wiener_log_survival(c, x0 - c.tau) * c.valid;
        return wiener_logpdf<MODEL>(c, x0, x1 > 0.0f ? 1 : 0) + (x1 == x1 ? 0.0f : x1);
    } else {                                                            // (y, acc): rt = |y|, upper iff y > 0; y == 0 has no time
        const float r = wiener_logpdf<MODEL>(c, fabsf(x0), x0 > 0.0f ? 1 : 0);
        return x0 == 0.0f ? __builtin_nanf("") : r;
    }
}

// Lane k's value as a wave-uniform one.  The kernels broadcast a struct of floats word by word with a loop written out in place: the same
// loop as a function (by value, by reference or through a bit cast) cost the forward basic kernels 4 VGPRs and a wave per SIMD, and the
// gradient kernels 8 to 14 VGPRs and a wave per SIMD (profiles/r21_wiener_sweep_resources.txt).
__device__ __forceinline__ float wiener_bcast(float x, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), k)); }

// The rows [rbase, rend) of workgroup blockIdx.x, ROWS at most.  STAGED (broadcast layout): the `chunks` workgroups of a data set split
// its S rows, the last one ragged; else (paired layout) the workgroups split all R rows.  The one mapping of the family's kernels.
template <bool STAGED, int ROWS>
__device__ __forceinline__ void wiener_block_rows(long long R, long long S, long long chunks, long long &rbase, long long &rend)
{
    if (STAGED) {
        const long long d = blockIdx.x / chunks, ch = blockIdx.x - d * chunks;
        rbase = d * S + ch * ROWS;
        rend = rbase + ROWS < (d + 1) * S ? rbase + ROWS : (d + 1) * S;
    } else {
        rbase = (long long)blockIdx.x * ROWS;
        rend = rbase + ROWS < R ? rbase + ROWS : R;
    }
}

// The workgroup's 256 threads stage nt <= WIENER_TILE pairs of its data set in LDS; every thread of the workgroup calls it
__device__ __forceinline__ void wiener_stage_tile(float2 *tile, const float *src, int nt)
{
    __syncthreads();                                                   // the previous tile is no longer read
    for (int j = threadIdx.x; j < nt; j += 256) tile[j] = make_float2(src[2 * j], src[2 * j + 1]);
    __syncthreads();
}

// The pairs of row `row`'s data set from trial t0 on
__device__ __forceinline__ const float *wiener_pairs(const float *data, long long S, int N, long long row, int t0)
{
    return data + ((row / S) * (long long)N + t0) * 2;
}

// The one row of wave `wave`, for the kernels that give a wave one row and a workgroup ROWS = 4.  A wave without a row (the ragged last
// workgroup) has nothing to do in the paired layout and returns; in the broadcast layout it still stages, so it goes on with the last
// row's constants (`row` is clamped into range) and `has_row` keeps it from scoring and storing.
struct WienerWaveRow {
    long long rbase, row;
    bool has_row;               // wave-uniform
};
template <bool STAGED, int ROWS>
__device__ __forceinline__ WienerWaveRow wiener_wave_row(long long R, long long S, long long chunks, int wave)
{
    long long rbase, rend;
    wiener_block_rows<STAGED, ROWS>(R, S, chunks, rbase, rend);
    WienerWaveRow w;
    w.rbase = rbase;
    w.has_row = rbase + wave < rend;
    w.row = w.has_row ? rbase + wave : rend - 1;
    return w;
}

// The head of a kernel's tile loop, `for (int t0 = 0; t0 < N; t0 += WIENER_TILE)`: the number of trials nt <= WIENER_TILE of the tile
// that begins at t0, after the workgroup has staged them (STAGED: every thread of the workgroup gets here; rbase tells the data set)
// A data set may hold fewer trials than its stride: the sweep is over `n` <= N trials of a set whose rows lie N pairs apart (the ragged
// marginal kernel; n must be workgroup-uniform when STAGED, the staging barrier is every thread's).  The others sweep all N.
template <bool STAGED>
__device__ __forceinline__ int wiener_enter_tile(float2 *tile, const float *data, long long S, int N, int n, long long rbase, int t0)
{
    const int nt = n - t0 < WIENER_TILE ? n - t0 : WIENER_TILE;
    if (STAGED) wiener_stage_tile(tile, wiener_pairs(data, S, N, rbase, t0), nt);
    return nt;
}
template <bool STAGED>
__device__ __forceinline__ int wiener_enter_tile(float2 *tile, const float *data, long long S, int N, long long rbase, int t0)
{
    return wiener_enter_tile<STAGED>(tile, data, S, N, N, rbase, t0);
}

// A lane's pairs of one row in one tile: f(i, x0, x1) for the trials t0 + i, i = lane, lane + 64, ... below nt, in that order.
// STAGED: from the staged tile; else from the row's own data set in HBM, and with PREFETCH the next pair is loaded before this one is
// evaluated, so that HBM latency overlaps the arithmetic.
template <bool STAGED, bool PREFETCH, class F>
__device__ __forceinline__ void wiener_tile_trials(const float2 *tile, const float *data, long long S, int N, long long row, int t0, int nt, int lane,
                                                   const F &f)
{
    const float *src = STAGED ? nullptr : wiener_pairs(data, S, N, row, t0);
    float n0 = 0.0f, n1 = 0.0f;
    if (!STAGED && PREFETCH && lane < nt) { n0 = src[2 * lane]; n1 = src[2 * lane + 1]; }
    for (int i = lane; i < nt; i += 64) {
        float x0, x1;
        if (STAGED) { const float2 x = tile[i]; x0 = x.x; x1 = x.y; }
        else if (PREFETCH) {
            x0 = n0; x1 = n1;
            if (i + 64 < nt) { n0 = src[2 * (i + 64)]; n1 = src[2 * (i + 64) + 1]; }
        } else { x0 = src[2 * i]; x1 = src[2 * i + 1]; }
        f(i, x0, x1);
    }
}

// The whole sweep of a wave's one row: every tile staged by all, and f(t, x0, x1) for the lane's trials t = lane, lane + 64, ... below N
// in the waves that have a row.  With a sweep length `n` of its own: the trials below n <= N of a set N pairs long (wiener_enter_tile).
template <bool STAGED, bool PREFETCH, class F>
__device__ __forceinline__ void wiener_row_trials(float2 *tile, const float *data, long long S, int N, int n, const WienerWaveRow &w, int lane,
                                                  const F &f)
{
    for (int t0 = 0; t0 < n; t0 += WIENER_TILE) {
        const int nt = wiener_enter_tile<STAGED>(tile, data, S, N, n, w.rbase, t0);
        if (w.has_row) wiener_tile_trials<STAGED, PREFETCH>(tile, data, S, N, w.row, t0, nt, lane, [&](int i, float x0, float x1) { f(t0 + i, x0, x1); });
    }
}
template <bool STAGED, bool PREFETCH, class F>
__device__ __forceinline__ void wiener_row_trials(float2 *tile, const float *data, long long S, int N, const WienerWaveRow &w, int lane, const F &f)
{
    wiener_row_trials<STAGED, PREFETCH>(tile, data, S, N, N, w, lane, f);
}

// The sum of the 64 lanes' values in the butterfly's order (a + b == b + a: every lane ends with the same bits)
__device__ __forceinline__ double wiener_wave_sum(double s)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m, 64);
    return s;
}

// STAGED: the workgroup's rows all score one data set, read from LDS (broadcast layout); else every row reads its own (paired layout)
template <int MODEL, bool STAGED>
__global__ __launch_bounds__(256) void wiener_kernel(WienerArgs A)
{
    __shared__ float2 tile[STAGED ? WIENER_TILE : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long rbase, rend;
    wiener_block_rows<STAGED, WIENER_ROWS>(A.R, A.S, A.chunks, rbase, rend);
    const long long wrow0 = rbase + wave;                               // the wave's rows: wrow0 + 4k, k < WIENER_RPW
    const bool has_rows = wrow0 < rend;
    if (!STAGED && !has_rows) return;
    // lane k < WIENER_RPW works out the constants of the wave's k-th row (clamped into range; unused lanes repeat the last)
    WienerRow mine;
    {
        long long r = wrow0 + 4ll * (lane < WIENER_RPW ? lane : WIENER_RPW - 1);
        if (r >= rend) r = rend - 1;
        if (r < rbase) r = rbase;
        mine = wiener_row<MODEL>(A.params + r * A.P);
    }
    // per-lane partial sums of the wave's rows (named, not an array: the row loop is not unrolled, and a dynamically indexed array
    // would live in scratch)
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    static_assert(WIENER_RPW == 4, "one partial sum per row of the wave");
    for (int t0 = 0; t0 < A.N; t0 += WIENER_TILE) {
        const int nt = wiener_enter_tile<STAGED>(tile, A.data, A.S, A.N, rbase, t0);       // (staged once for the wave's four rows)
#pragma nounroll
        for (int k = 0; k < WIENER_RPW; ++k) {
            const long long row = wrow0 + 4ll * k;
            if (row >= rend) break;                                     // wave-uniform
            WienerRow c;
            const float *m = reinterpret_cast<const float *>(&mine);
            float *cw = reinterpret_cast<float *>(&c);
#pragma unroll
            for (int f = 0; f < WIENER_ROW_WORDS; ++f) cw[f] = wiener_bcast(m[f], k);
            float *dst = A.out_trial ? A.out_trial + row * (long long)A.N + t0 : nullptr;
            double s = k == 0 ? acc0 : k == 1 ? acc1 : k == 2 ? acc2 : acc3;
            wiener_tile_trials<STAGED, true>(tile, A.data, A.S, A.N, row, t0, nt, lane, [&](int i, float x0, float x1) {
                const float lf = wiener_trial<MODEL>(c, x0, x1);
                if (dst) dst[i] = lf;
                s += (double)lf;
            });
            acc0 = k == 0 ? s : acc0; acc1 = k == 1 ? s : acc1; acc2 = k == 2 ? s : acc2; acc3 = k == 3 ? s : acc3;
        }
    }
    if (!A.out_sum || !has_rows) return;
    for (int k = 0; k < WIENER_RPW; ++k) {
        const long long row = wrow0 + 4ll * k;
        if (row >= rend) break;
        const double s = wiener_wave_sum(k == 0 ? acc0 : k == 1 ? acc1 : k == 2 ? acc2 : acc3);
        if (lane == 0) A.out_sum[row] = s;
    }
}

}  // namespace nddm
