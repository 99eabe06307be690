// nddm_wiener_grad.h -- value and gradient of the batched Wiener first-passage log-likelihood (gfx950): what a gradient-based fit
// consumes per step (Stan's NUTS over wiener_lpdf; MAP refinement, Laplace / variational fits, HMC or MALA on many data sets at
// once), one fused launch.  Included by nddm_kernels.hip (one translation unit) after nddm_wiener.h, whose wiener_row / wiener_logpdf /
// wiener_trial give the value unchanged.  DESIGN.md section 14.
//
// Natural coordinates (nddm_wiener.h): lower-boundary form, t = rt - tau, a', w, nu', eta', u = t / a'^2, D = 1 + eta'^2 t.  With
//     M = (a' w + nu' t) / D          (minus the derivative in nu')          K = nu' - eta'^2 M      (the drift the path "saw")
// the drift term (eta'^2 a'^2 w^2 - 2 a' nu' w - nu'^2 t) / (2D) - 1/2 log D = eta'^2 (a' w + nu' t)^2 / (2D) - a' nu' w - nu'^2 t / 2 - 1/2 log D
// differentiates in closed form, and with Gu = d/du log g, Gw = d/dw log g:
//     d/dt    = Gu / a'^2 - K^2 / 2 - eta'^2 / (2D)
//     d/da'   = -2 (u Gu + 1) / a' - w K
//     d/dw    = Gw - a' K
//     d/dnu'  = -M
//     d/deta' = eta' (M^2 - t / D)
// (eta = 0: D = 1, K = nu', M = a' w + nu' t: the derivatives of the plain -a' nu' w - nu'^2 t / 2.)  log g's partials are ratios of sums
// over the exponentials the density already forms, with E_k = exp(-((w + 2k)^2 - w^2) / (2u)) = 1, A, B, A^3 B, A B^3 for k = 0, -1, 1, -2, 2:
//     small time  Gu = -3 / (2u) + sum (w + 2k)^3 E_k / (2 u^2 sum (w + 2k) E_k)        Gw = sum (1 - (w + 2k)^2 / u) E_k / sum (w + 2k) E_k
//     large time  Gu = -(pi^2 / 2) sum k^3 sin(k pi w) q^(k^2) / sum k sin(k pi w) q^(k^2)
//                 Gw = pi sum k^2 cos(k pi w) q^(k^2) / sum k sin(k pi w) q^(k^2),   k = 1..3
// the large-time ones with sin(k pi w) / sin(pi w) = 1, 2c, 4c^2 - 1 and cos(k pi w) = c, 2c^2 - 1, 4c^3 - 3c from the row's c = cos(pi w):
// no new sin / cos per trial.  The same per-lane select at WIENER_U_STAR, the same fixed trips (their truncation error in the partials is
// below 1e-8: tests/test_wiener_grad_host.py); the denominators are the density's own sums, so beyond the density's transcendentals a
// trial costs ONE v_rcp_f32, the reciprocal of the selected sum.
//
// The side: the upper boundary is the lower-boundary form at (-nu', 1 - beta), so a trial adds its nu' and w partials with the side's
// sign and the row's sums are in (t, a', beta, v', eta').  Chain rule, once per row, in float64, after the reduction: d/dtau = -d/dt;
// a' = a / s, v' = v / s, eta' = eta / s give d/da = (d/da') / s, d/dv = (d/dv') / s, d/deta = (d/deta') / s and
// d/ds = -(a' d/da' + v' d/dv' + eta' d/deta') / s.  alpha_not_scaled's Nu is clipped to +-5 (wiener_row): where the clip is active
// d/dNu = 0, the derivative of the clamp, and the other columns are those of the clipped value.
//
// Special values (the math, none an error): an invalid row (wiener_row's conditions) gives NaN in the value and in every gradient column,
// its neighbours unaffected; a trial with t <= 0 gives -inf in the value, as the density does, and NaN in every gradient column of its
// row; alpha_not_scaled's y == 0 gives NaN in both.
//   basic_ddm_dc's censored timeouts (choice 0): the VALUE scores them exactly as wiener_kernel does (wiener_log_survival), so the row's
//   log-likelihood is unchanged.  The GRADIENT is opt-in (NDDM_WIENER_CENSORED, the CENSORED instantiations): without the flag a row with a
//   censored trial gets NaN in every gradient column, never a partial gradient that silently leaves the censored trials out (done by
//   poisoning the row's sums; the value's summation order does not change).  With it a censored trial adds the partials of
//   log S(t; a', w, v') to the same sums: d/da', d/dw, d/dv' from wiener_log_survival_grad (nddm_wiener_survival_grad.h, both forms, the
//   value's select) and d/dt = -(f_lower + f_upper) / S (wiener_grad_censored), so d/dtau = +(f_lower + f_upper) / S through the row's chain
//   rule.  A censored trial with t <= 0 is log 1 = 0 with zero partials; a non-finite rt or a choice other than 1, -1, 0 poisons the row.
//   The value is wiener_trial's in either case, bit for bit.
//
// Execution: the two layouts and the dispatch rule of wiener_kernel (broadcast, the data set staged in LDS one WIENER_TILE at a time,
// when draws_per_dataset >= WIENER_ROWS; paired otherwise).  Six float64 partial sums per row do not fit four rows per wave in the
// register budget, so a wave owns WIENER_GRAD_RPW = 1 row and a workgroup of 4 waves WIENER_GRAD_ROWS = 4 consecutive ones.  Lane j
// accumulates trials j, j + 64, ... of the row in that order in float64 -- the value in exactly wiener_kernel's order, so the row's
// log-likelihood has the same bits as nddm_wiener_log_likelihood's -- a butterfly of the 64 partial sums reduces each of the six, and lane 0
// applies the chain rule and stores.  The bits are a function of (the row's parameters, its data set, n_trials) alone: not of the layout,
// the grid, the stream or a capture.  No scratch memory, no atomics; stores are plain vector stores.
#pragma once
#include "nddm_wiener.h"
#include "nddm_wiener_survival_grad.h"

namespace nddm {

constexpr int WIENER_GRAD_RPW = 1;                          // rows per wave
constexpr int WIENER_GRAD_ROWS = 4 * WIENER_GRAD_RPW;       // rows per workgroup (4 waves)

struct WienerGradArgs {
    const float *params;        // [R, P]
    const float *data;          // [D, N, 2]
    double *out_sum;            // [R] or NULL
    double *out_grad;           // [R, P]
    long long R, S;             // rows, rows per data set
    long long chunks;           // workgroups per data set (broadcast layout)
    int N, P;
};

// What the gradient needs of a row beyond WienerRow (a struct of its own: wiener_kernel's registers do not change)
struct WienerGradRow {
    float a2, ia;               // a'^2, 1 / a'
    float ep;                   // eta'
    float g0, g1, g2;           // pi c / s, 4 pi (2c^2 - 1) / s, 9 pi (4c^3 - 3c) / s with c = cos(pi beta), s = sin(pi beta): the lower
                                // boundary's; the upper one's (c -> -c) are -g0, g1, -g2
};
constexpr int WIENER_GRAD_ROW_WORDS = sizeof(WienerGradRow) / sizeof(float);

// (the parameters exactly as wiener_row reads and clips them)
template <int MODEL>
__device__ __forceinline__ WienerGradRow wiener_grad_row(const float *p, const WienerRow &c)
{
    const float eta = MODEL == NDDM_BASIC_DDM_DC ? 0.0f : p[4], s = MODEL == NDDM_BASIC_DDM_DC ? p[4] : p[5];
    WienerGradRow g;
    g.a2 = c.ap * c.ap;
    g.ia = 1.0f / c.ap;
    g.ep = eta / s;
    const float cb = c.cpb, pis = 3.14159265358979324f / c.s1;
    g.g0 = pis * cb;
    g.g1 = 4.0f * pis * (2.0f * (cb * cb) - 1.0f);
    g.g2 = 9.0f * pis * (cb * (4.0f * (cb * cb) - 3.0f));
    return g;
}

// A lane's partial sums of one row: the value and the partials in (t, a', beta, v', eta'); `poison` is 0 or NaN and joins the five
// gradient sums before the reduction (a censored trial, t <= 0, a NaN in the data)
struct WienerGradAcc {
    double v, t, a, w, nu, eta;
    float poison;
};

__device__ __forceinline__ WienerGradAcc wiener_grad_zero()
{
    WienerGradAcc s;
    s.v = s.t = s.a = s.w = s.nu = s.eta = 0.0;
    s.poison = 0.0f;
    return s;
}

// A lane's `poison` into its gradient sums, never into the value (basic_ddm_dc has no eta column: that sum stays 0).  The one place that
// says which sums are poisoned: the kernels, the sampler's host build and the host tools all call it.
template <int MODEL>
__device__ __forceinline__ void wiener_grad_fold(WienerGradAcc &s)
{
    const double poison = (double)s.poison;
    s.t += poison; s.a += poison; s.w += poison; s.nu += poison;
    if (MODEL != NDDM_BASIC_DDM_DC) s.eta += poison;
}

// The fold, then every sum over the wave: every lane ends with the row's sums.  (wiener_wave_sum's butterfly with the sums side by side in
// each step: as one wiener_wave_sum per sum the gradient kernels measured 0.6 to 1.2 % slower, profiles/r21_wiener_sweep_ab.txt.)
template <int MODEL>
__device__ __forceinline__ void wiener_grad_reduce(WienerGradAcc &s)
{
    wiener_grad_fold<MODEL>(s);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {                                  // a + b == b + a: every lane ends with the same bits
        s.v += __shfl_xor(s.v, m, 64);
        s.t += __shfl_xor(s.t, m, 64);
        s.a += __shfl_xor(s.a, m, 64);
        s.w += __shfl_xor(s.w, m, 64);
        s.nu += __shfl_xor(s.nu, m, 64);
        if (MODEL != NDDM_BASIC_DDM_DC) s.eta += __shfl_xor(s.eta, m, 64);
    }
}

// A censored timeout of basic_ddm_dc (choice 0 at response time rt) into a lane's gradient sums: the partials of log S(t; a', w, v') at
// t = rt - tau.  a', w = beta and v' are wiener_log_survival_grad's; d/dt log S = -(f_lower(t) + f_upper(t)) / S(t) is formed as
// -(e^{log f_lower - log S} + e^{log f_upper - log S}) from wiener_logpdf's two values and the same log S: exact (no second series to
// truncate), it cannot overflow where S is small, and at large t it tends to lambda_1 as it must.  t <= 0 is log 1 = 0 with zero partials,
// not a poison; a non-finite rt poisons the row.  (The value has already been added by the caller: wiener_trial's.)
__device__ __forceinline__ void wiener_grad_censored(const WienerRow &c, float rt, WienerGradAcc &s)
{
    const float t = rt - c.tau;
    if (t > 0.0f) {
        const WienerSurvivalGrad h = wiener_log_survival_grad(c, t);
        const float fl = wiener_logpdf<NDDM_BASIC_DDM_DC>(c, rt, 0), fu = wiener_logpdf<NDDM_BASIC_DDM_DC>(c, rt, 1);
        const float haz = __expf(fminf(fl - h.ls, 80.0f)) + __expf(fminf(fu - h.ls, 80.0f));
        s.t -= (double)haz;
        s.a += (double)h.da;
        s.w += (double)h.dw;
        s.nu += (double)h.dv;
    }
    s.poison += fabsf(rt) < __builtin_inff() ? 0.0f : __builtin_nanf("");
}

// One trial into a lane's sums.  The value is wiener_trial's; the partials repeat the density's expressions for A, B, q and the two sums
// so that the compiler shares them.  CENSORED (basic_ddm_dc, NDDM_WIENER_CENSORED): a choice-0 trial adds the partials of log S
// (wiener_grad_censored) and any choice other than 1, -1 and 0 poisons the row; the branch is taken by the lanes that hold a timeout, so
// a sweep in which no lane holds one skips the survival code as a wave.  Without it a choice-0 trial poisons the row, and the
// instantiation holds none of the survival code.
template <int MODEL, bool CENSORED = false>
__device__ __forceinline__ void wiener_grad_trial(const WienerRow &c, const WienerGradRow &g, float x0, float x1, WienerGradAcc &s)
{
    static_assert(!CENSORED || MODEL == NDDM_BASIC_DDM_DC, "only basic_ddm_dc's timeouts carry a time");
    s.v += (double)wiener_trial<MODEL>(c, x0, x1);
    if (CENSORED && x1 == 0.0f) {
        wiener_grad_censored(c, x0, s);
        return;
    }
    float rt;
    int sd;
    bool bad;
    if (MODEL == NDDM_BASIC_DDM_DC) {                                   // without CENSORED a timeout has no gradient here
        rt = x0; sd = x1 > 0.0f ? 1 : 0;
        bad = CENSORED ? !(x1 == 1.0f || x1 == -1.0f) : x1 == 0.0f || x1 != x1;
    }
    else { rt = fabsf(x0); sd = x0 > 0.0f ? 1 : 0; bad = false; }                                          // (y == 0: t = -tau <= 0)
    const float t = rt - c.tau;
    bad = bad || !(t > 0.0f);
    const float w = sd ? c.w[1] : c.w[0];
    const float nu = sd ? -c.vp : c.vp;
    const float tc = fmaxf(t, 1.17549435e-38f);
    const float it = __builtin_amdgcn_rcpf(tc);
    // small time: sums of 1, x^2 and x^3 over E_k beside the density's sum of x, x = w + 2k
    const float A = __builtin_amdgcn_exp2f((sd ? c.m1[1] : c.m1[0]) * it);
    const float B = __builtin_amdgcn_exp2f((sd ? c.m2[1] : c.m2[0]) * it);
    const float A3B = (A * A) * (A * B), AB3 = (B * B) * (A * B);
    const float ssum = w + (w - 2.0f) * A + (w + 2.0f) * B + (w - 4.0f) * A3B + (w + 4.0f) * AB3;
    const float xa = w - 2.0f, xb = w + 2.0f, xc = w - 4.0f, xd = w + 4.0f;
    const float w2 = w * w, xa2 = xa * xa, xb2 = xb * xb, xc2 = xc * xc, xd2 = xd * xd;
    const float T0 = 1.0f + A + B + A3B + AB3;
    const float T2 = w2 + xa2 * A + xb2 * B + xc2 * A3B + xd2 * AB3;
    const float S3 = w2 * w + (xa2 * xa) * A + (xb2 * xb) * B + (xc2 * xc) * A3B + (xd2 * xd) * AB3;
    // large time: sums of k^3 sin and k^2 cos beside the density's sum of k sin, sin(pi w) and q taken out
    const float q = __builtin_amdgcn_exp2f(c.mq * t);
    const float q2 = q * q, q4 = q2 * q2, q3 = q2 * q, q8 = q4 * q4;
    const float c4 = sd ? c.c4[1] : c.c4[0], c3 = sd ? c.c3[1] : c.c3[0];
    const float lsum = 1.0f + c4 * q3 + c3 * q8;
    const float L3 = 1.0f + (4.0f * c4) * q3 + (9.0f * c3) * q8;
    const float LW = (sd ? -g.g0 : g.g0) + g.g1 * q3 + (sd ? -g.g2 : g.g2) * q8;
    const bool small = t < c.tstar;
    const float rS = __builtin_amdgcn_rcpf(small ? ssum : lsum);       // the one transcendental the gradient adds
    const float ai = g.a2 * it;                                         // 1 / u
    const float ugu_s = 0.5f * ai * (S3 * rS) - 1.5f;                   // u Gu
    const float gt_l = c.lq * (L3 * rS);                                // Gu / a'^2
    const float gt = small ? it * ugu_s : gt_l;
    const float ugu = small ? ugu_s : t * gt_l;
    const float gw = small ? (T0 - ai * T2) * rS : LW * rS;
    // the drift term
    float M = c.ap * w + nu * t, K = nu, eD = 0.0f, tD = t;
    if (MODEL == NDDM_ALPHA_NOT_SCALED && c.e2 > 0.0f) {                // (row-uniform, as the density's branch)
        const float iD = __builtin_amdgcn_rcpf(1.0f + c.e2 * t);
        M = M * iD;
        K = nu - c.e2 * M;
        eD = c.e2 * iD;
        tD = t * iD;
    }
    const float pt = gt - 0.5f * (K * K) - 0.5f * eD;
    const float pa = -2.0f * g.ia * (ugu + 1.0f) - w * K;
    const float pw = gw - c.ap * K;
    s.t += (double)pt;
    s.a += (double)pa;
    s.w += (double)(sd ? -pw : pw);
    s.nu += (double)(sd ? M : -M);
    if (MODEL != NDDM_BASIC_DDM_DC) s.eta += (double)(g.ep * (M * M - tD));    // (basic_ddm_dc has no eta column)
    s.poison += bad ? __builtin_nanf("") : 0.0f;
}

// The row's six sums -> its log-likelihood and its gradient in the model's parameter columns (float64; lane 0 of the kernel)
template <int MODEL>
__device__ __forceinline__ void wiener_grad_finish(const float *p, float valid, const WienerGradAcc &s, double *out_sum, double *out_grad)
{
    if (out_sum) *out_sum = s.v;
    float v = p[0];
    const float a = p[1], eta = MODEL == NDDM_BASIC_DDM_DC ? 0.0f : p[4], sc = MODEL == NDDM_BASIC_DDM_DC ? p[4] : p[5];
    bool clipped = false;
    if (MODEL == NDDM_ALPHA_NOT_SCALED && (v < -5.0f || v > 5.0f)) { v = v > 0.0f ? 5.0f : -5.0f; clipped = true; }
    const double is = 1.0 / (double)sc, nan = (double)valid;           // valid: 1 or NaN
    const double ap = (double)a * is, vp = (double)v * is, ep = (double)eta * is;
    const double dv = s.nu * is, da = s.a * is, de = s.eta * is, dsc = -(ap * s.a + vp * s.nu + ep * s.eta) * is;
    out_grad[0] = (clipped && dv == dv ? 0.0 : dv) * nan;               // (a poisoned row stays NaN where Nu is clipped)
    out_grad[1] = da * nan;
    out_grad[2] = s.w * nan;
    out_grad[3] = -s.t * nan;
    if (MODEL == NDDM_BASIC_DDM_DC) out_grad[4] = dsc * nan;
    else { out_grad[4] = de * nan; out_grad[5] = dsc * nan; }
}

// STAGED: the workgroup's rows all score one data set, read from LDS (broadcast layout); else every row reads its own (paired layout).
// CENSORED: wiener_grad_trial's switch (NDDM_WIENER_CENSORED); the instantiations without it are the kernels as they were.
template <int MODEL, bool STAGED, bool CENSORED = false>
__global__ __launch_bounds__(256) void wiener_grad_kernel(WienerGradArgs G)
{
    __shared__ float2 tile[STAGED ? WIENER_TILE : 1];
    static_assert(WIENER_GRAD_RPW == 1, "a wave holds one row's six partial sums");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WienerWaveRow w = wiener_wave_row<STAGED, WIENER_GRAD_ROWS>(G.R, G.S, G.chunks, wave);
    if (!STAGED && !w.has_row) return;
    const float *p = G.params + w.row * G.P;
    // every lane works out the row's constants; the wave keeps lane 0's copy as uniform values
    WienerRow c;
    WienerGradRow g;
    {
        const WienerRow mine = wiener_row<MODEL>(p);
        const WienerGradRow gmine = wiener_grad_row<MODEL>(p, mine);
        const float *m = reinterpret_cast<const float *>(&mine), *gm = reinterpret_cast<const float *>(&gmine);
        float *cw = reinterpret_cast<float *>(&c), *gw = reinterpret_cast<float *>(&g);
#pragma unroll
        for (int f = 0; f < WIENER_ROW_WORDS; ++f) cw[f] = wiener_bcast(m[f], 0);
#pragma unroll
        for (int f = 0; f < WIENER_GRAD_ROW_WORDS; ++f) gw[f] = wiener_bcast(gm[f], 0);
    }
    WienerGradAcc s = wiener_grad_zero();
    // wiener_row_trials<STAGED, true>, written out: with the trial as a functor this kernel's alpha_not_scaled broadcast launch measured 1 %
    // slower than with the loop in place (profiles/r21_wiener_sweep_ab.txt), so here the sweep is its own copy of wiener_tile_trials' loop
    for (int t0 = 0; t0 < G.N; t0 += WIENER_TILE) {
        const int nt = wiener_enter_tile<STAGED>(tile, G.data, G.S, G.N, w.rbase, t0);
        if (!w.has_row) continue;
        const float *src = STAGED ? nullptr : wiener_pairs(G.data, G.S, G.N, w.row, t0);
        float n0 = 0.0f, n1 = 0.0f;
        if (!STAGED && lane < nt) { n0 = src[2 * lane]; n1 = src[2 * lane + 1]; }
        for (int i = lane; i < nt; i += 64) {
            float x0, x1;
            if (STAGED) { const float2 x = tile[i]; x0 = x.x; x1 = x.y; }
            else {
                x0 = n0; x1 = n1;
                if (i + 64 < nt) { n0 = src[2 * (i + 64)]; n1 = src[2 * (i + 64) + 1]; }
            }
            wiener_grad_trial<MODEL, CENSORED>(c, g, x0, x1, s);
        }
    }
    if (!w.has_row) return;
    wiener_grad_reduce<MODEL>(s);
    if (lane == 0) wiener_grad_finish<MODEL>(p, c.valid, s, G.out_sum ? G.out_sum + w.row : nullptr, G.out_grad + w.row * G.P);
}

}  // namespace nddm
