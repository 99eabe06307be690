// nddm_wiener_marginal_grad.h -- value and gradient of the single-trial model's marginal log-likelihood (NDDM_SINGLE_TRIAL): what a
// gradient-based fit of the reference's headline model consumes per step (MAP refinement of amortized draws, Laplace / variational fits,
// HMC / NUTS), one fused launch.  Included by nddm_kernels.hip (one translation unit) after nddm_wiener_marginal.h, whose
// wiener_marginal_row / wiener_marginal_node give the value unchanged, and nddm_wiener_grad.h, whose formulas for the partials of log f
// are evaluated here at eta = 0.  DESIGN.md section 16.
//
// The quantity, in nddm_wiener_marginal.h's notation: one trial has
//     log L = log N(z; gamma mu, s2m) - log Phi(mu / sd) + log int e^{l(x)} dx,
//     l(x)  = log h(t, a' = e^x / dc, v', w) + x - (e^x - m)^2 / (2 tau^2) - log tau - 1/2 log(2 pi).
// The integral's limits are wherever the integrand is negligible, so d/dtheta log int is the expectation of d/dtheta l under the normalised
// integrand: sum_k W_k dl_k / sum_k W_k over the LAST pass's 32 nodes, W_k = w_k e^{l_k - shift}; the zoom windows are not differentiated.
// Per node the partials are Ht = d/dt log h, a' Ha = d/dx log h, Hw = d/dbeta log h, Hv = d/dv' log h, (a - m) / tau^2 (= d/dm) and
// (a - m)^2 / tau^3 - 1 / tau (= d/dtau).
//   A response: Ht, Ha, Hw, Hv are nddm_wiener_grad.h's at eta' = 0 (M = a' w + nu' t, K = nu'); the upper boundary is the lower form at
//   (-nu', 1 - w), its w and nu' partials with the side's sign.
//   A timeout: Ht = 0 (t_censor is a constant of the call); Ha, Hw, Hv are the partials of log S at fixed t, wiener_log_survival_grad
//   (nddm_wiener_survival_grad.h, which nddm_wiener_grad.h includes: basic_ddm_dc's censored rows call the same function).
//
// Where the partials live: in a RE-WALK of the last pass's 32 nodes, merged with the value's own log-sum-exp loop.  The three passes are
// wiener_marginal_trial's, statement by statement, and leave the last pass's l_k in LDS; the loop that sums w_k e^{l_k - M} for the value
// (the same fmaf chain: the value has the forward kernel's bits -- tests/test_wiener_marginal_grad_host.py holds the two equal bit for bit on
// the host, tests/test_gpu_wiener_marginal_grad.py on the device) also evaluates the node's partials -- the density's exponentials again,
// not its logarithms -- and adds W_k times each into six float32 numerators; the denominator is the value's sum itself.  The shift is the
// last pass's own maximum, so no weight exceeds w_k.  A node whose weight has underflowed adds nothing (its partials may be infinite
// there).  Accumulating on the fly inside the last pass (pass 2's maximum as the shift) saves those exponentials but keeps the node's and
// the partials' values live together with the six numerators: it compiled to 150 VGPRs against this form's.
//
// Chain rule, once per row, in float64, after the reduction (lane 0): d/ddrift = sum Hv / dc, d/dbeta = sum Hw, d/dter = -sum Ht,
// d/ddc = -sum (a' Ha + v' Hv) / dc; mu, sd, sigma1 and gamma reach the result through m = k0 + k1 z and tau -- the row sums of E[a - m],
// z E[a - m] and E[(a - m)^2] -- and through the closed-form terms outside the integral -- sum dz, sum dz^2 (dz = z - gamma mu), the
// trial count and the inverse Mills ratio phi / Phi (mu / sd), formed from erfcx below 0 so that it keeps its digits.
//
// Special values (the math, none an error): an invalid row (wiener_marginal_row's conditions) gives NaN in the value and in every column,
// its neighbours unaffected; a response with |y| <= ter gives -inf in the value and NaN in every column of its row; a timeout with
// t_censor <= 0 (or NaN), a non-finite z1 or a NaN y give NaN in both; every node at -inf gives -inf and NaN.  A valid row of valid trials,
// TIMEOUTS INCLUDED, gets a finite gradient.  A per-lane 0 / NaN float (`poison`) joins the gradient sums before the reduction: the order
// of summation never changes.
//
// Execution: wiener_marginal_kernel's.  A wave owns one row, a workgroup of 4 waves WMGRAD_ROWS = 4 consecutive ones; broadcast layout
// when draws_per_dataset >= WIENER_ROWS, paired otherwise.  Lane j accumulates trials j, j + 64, ... in float64 -- the value in exactly
// wiener_marginal_kernel's order -- a butterfly reduces each of the ten sums and lane 0 applies the chain rule and stores.  The bits are a
// function of (the row's parameters, its data set, n_trials, t_censor) alone.  A pass's node values live in LDS as in the forward kernel
// (32 KB per workgroup); no scratch memory, no atomics; stores are plain vector stores.
#pragma once
#include "nddm_wiener_grad.h"
#include "nddm_wiener_marginal.h"

namespace nddm {

constexpr int WMGRAD_RPW = 1;                   // rows per wave
constexpr int WMGRAD_ROWS = 4 * WMGRAD_RPW;     // rows per workgroup (4 waves)
constexpr int WMGRAD_COLS = 8;                  // drift, mu_alpha, beta, ter, std_alpha, dc, sigma1, gamma

struct WienerMarginalGradArgs {
    const float *params;        // [R, 8]
    const float *data;          // [D, N, 2] = (choicert, z1)
    double *out_sum;            // [R] or NULL
    double *out_grad;           // [R, 8]
    long long R, S;             // rows, rows per data set
    long long chunks;           // workgroups per data set (broadcast layout)
    int N, P;
    float t_censor;
};

// (The side is read behind an empty asm per node: without it the compiler hoists every side-selected row constant and its products out
// of the node loop into vector registers that stay live through the whole loop, and the kernel loses waves.)
#if defined(__HIP_DEVICE_COMPILE__)
#define WMGRAD_PER_NODE(a) asm volatile("" : "+v"(a))
#else
#define WMGRAD_PER_NODE(a) ((void)0)
#endif
// The partials of log h at a node: d/dt, a' d/da' (= d/dx), d/dbeta, d/dv'
struct WienerMarginalPartials {
    float ht, xa, hw, hv;
};

// The a' = 1 row rescaled to a' = e^la, as wiener_marginal_node does it (the same expressions: the compiler shares them)
__device__ __forceinline__ WienerRow wiener_marginal_rescaled(const WienerRow &b, float la)
{
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
    return c;
}

// A response: wiener_grad_trial's partials at eta' = 0 (g: wiener_grad_row of the a' = 1 row -- g0, g1, g2 depend on beta alone).
// A timeout: the partials of log S.
__device__ __forceinline__ WienerMarginalPartials wiener_marginal_node_partials(const WienerRow &b, const WienerMarginalRow &r, const WienerGradRow &g,
                                                                                float x, float t, bool censored, int sd)
{
    const WienerRow c = wiener_marginal_rescaled(b, x - r.ldc);
    WienerMarginalPartials o;
    if (censored) {
        const WienerSurvivalGrad s = wiener_log_survival_grad(c, t);
        o.ht = 0.0f; o.xa = c.ap * s.da; o.hw = s.dw; o.hv = s.dv;
        return o;
    }
    const float w = sd ? c.w[1] : c.w[0];
    const float nu = sd ? -c.vp : c.vp;
    const float tc = fmaxf(t, 1.17549435e-38f);
    const float it = __builtin_amdgcn_rcpf(tc);
    const float A = __builtin_amdgcn_exp2f((sd ? c.m1[1] : c.m1[0]) * it);
    const float B = __builtin_amdgcn_exp2f((sd ? c.m2[1] : c.m2[0]) * it);
    const float A3B = (A * A) * (A * B), AB3 = (B * B) * (A * B);
    const float ssum = w + (w - 2.0f) * A + (w + 2.0f) * B + (w - 4.0f) * A3B + (w + 4.0f) * AB3;
    const float xa = w - 2.0f, xb = w + 2.0f, xc = w - 4.0f, xd = w + 4.0f;
    const float w2 = w * w, xa2 = xa * xa, xb2 = xb * xb, xc2 = xc * xc, xd2 = xd * xd;
    const float T0 = 1.0f + A + B + A3B + AB3;
    const float T2 = w2 + xa2 * A + xb2 * B + xc2 * A3B + xd2 * AB3;
    const float S3 = w2 * w + (xa2 * xa) * A + (xb2 * xb) * B + (xc2 * xc) * A3B + (xd2 * xd) * AB3;
    const float q = __builtin_amdgcn_exp2f(c.mq * t);
    const float q2 = q * q, q4 = q2 * q2, q3 = q2 * q, q8 = q4 * q4;
    const float c4 = sd ? c.c4[1] : c.c4[0], c3 = sd ? c.c3[1] : c.c3[0];
    const float lsum = 1.0f + c4 * q3 + c3 * q8;
    const float L3 = 1.0f + (4.0f * c4) * q3 + (9.0f * c3) * q8;
    const float LW = (sd ? -g.g0 : g.g0) + g.g1 * q3 + (sd ? -g.g2 : g.g2) * q8;
    const bool small = t < c.tstar;
    const float rS = __builtin_amdgcn_rcpf(small ? ssum : lsum);
    const float ai = (c.ap * c.ap) * it;                                // 1 / u
    const float ugu_s = 0.5f * ai * (S3 * rS) - 1.5f;                   // u Gu
    const float gt_l = c.lq * (L3 * rS);                                // Gu / a'^2
    const float gt = small ? it * ugu_s : gt_l;
    const float ugu = small ? ugu_s : t * gt_l;
    const float gw = small ? (T0 - ai * T2) * rS : LW * rS;
    const float M = c.ap * w + nu * t;
    const float pw = gw - c.ap * nu;
    o.ht = gt - 0.5f * (nu * nu);
    o.xa = -2.0f * (ugu + 1.0f) - c.ap * (w * nu);
    o.hw = sd ? -pw : pw;
    o.hv = sd ? M : -M;
    return o;
}

// A lane's partial sums of one row: the value; the sums over its trials of E[Ht], E[a' Ha], E[Hw], E[Hv], E[a - m], z E[a - m],
// E[(a - m)^2], dz and dz^2; `poison` is 0 or NaN and joins the nine gradient sums before the reduction
struct WienerMarginalGradAcc {
    double v, t, a, w, nu, m1, zm, m2, dz, dz2;
    float poison;
};

__device__ __forceinline__ WienerMarginalGradAcc wiener_marginal_grad_zero()
{
    WienerMarginalGradAcc s;
    s.v = s.t = s.a = s.w = s.nu = s.m1 = s.zm = s.m2 = s.dz = s.dz2 = 0.0;
    s.poison = 0.0f;
    return s;
}

// A lane's `poison` into its nine gradient sums, never into the value: the one place that says which sums are poisoned (the kernel and
// the host tool both call it)
__device__ __forceinline__ void wiener_marginal_grad_fold(WienerMarginalGradAcc &s)
{
    const double poison = (double)s.poison;
    s.t += poison; s.a += poison; s.w += poison; s.nu += poison; s.m1 += poison; s.zm += poison; s.m2 += poison; s.dz += poison; s.dz2 += poison;
}

// The fold, then every sum over the wave: every lane ends with the row's sums (the sums side by side in each step of the butterfly, as
// wiener_grad_reduce has them and for its reason: one wiener_wave_sum per sum measured 1.2 % slower on the broadcast launch)
__device__ __forceinline__ void wiener_marginal_grad_reduce(WienerMarginalGradAcc &s)
{
    wiener_marginal_grad_fold(s);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {                                  // a + b == b + a: every lane ends with the same bits
        s.v += __shfl_xor(s.v, m, 64); s.t += __shfl_xor(s.t, m, 64); s.a += __shfl_xor(s.a, m, 64); s.w += __shfl_xor(s.w, m, 64);
        s.nu += __shfl_xor(s.nu, m, 64); s.m1 += __shfl_xor(s.m1, m, 64); s.zm += __shfl_xor(s.zm, m, 64); s.m2 += __shfl_xor(s.m2, m, 64);
        s.dz += __shfl_xor(s.dz, m, 64); s.dz2 += __shfl_xor(s.dz2, m, 64);
    }
}

// One trial into a lane's sums.  The window, the passes and the value are wiener_marginal_trial's, statement by statement; the last
// pass also accumulates the weighted partials (file header).  `gmd`: gamma mu in float64.
__device__ __forceinline__ void wiener_marginal_grad_trial(const WienerRow &b, const WienerMarginalRow &r, const WienerGradRow &g, double gmd, float y,
                                                           float z, float t_censor, float *buf, int stride, WienerMarginalGradAcc &s)
{
    const bool censored = y == 0.0f;
    const int sd = y > 0.0f ? 1 : 0;
    const float t0 = censored ? t_censor : fabsf(y) - r.ter;
    const bool dead = !(t0 > 0.0f);
    const bool zbad = !isfinite(z);
    const float t = dead ? 1.0f : fmaxf(t0, 1.0e-30f), zz = zbad ? 0.0f : z;
    const float m = fmaf(r.k1, zz, r.k0);
    const float st = sqrtf(t), vt = r.vp * t;
    const float c_lo = r.dc * st * 0.286788218175523f;
    const float mp = fmaxf(m, 0.0f), ltau = WMARG_L * r.tau;
    float hi;
    if (censored) {
        const float a1 = r.dc * fmaxf(fmaf(6.0f, st, vt) / (1.0f - r.beta), fmaf(6.0f, st, -vt) / r.beta);
        hi = fmaxf(mp, a1) + ltau;
    } else {
        const float w = sd ? 1.0f - r.beta : r.beta, nut = sd ? -vt : vt;
        hi = fmaxf(r.dc * (fmaxf(-nut, 0.0f) + st * 10.9544511501033f) / w, mp + ltau);
    }
    const bool below = m <= c_lo;
    const float mn = fminf(m, 0.0f);
    const float E = below ? ((c_lo - m) * (c_lo - m) - mn * mn) * r.i2t2 : 0.0f;
    const float D = st * 0.286788218175523f * fabsf(r.vp);
    float lo = c_lo * sqrtf(WMARG_CUT / (2.0f * WMARG_CUT + E + D));
    if (below) lo = fmaxf(lo, m - ltau);
    float xl = logf(fmaxf(lo, 1.0e-30f)), xh = logf(fminf(hi, 1.0e30f));
    float M = 0.0f, xr = 1.0f, xc = 0.0f, sum = 1.0f;
#pragma nounroll
    for (int pass = 0; pass < WMARG_PASSES; ++pass) {
        xc = 0.5f * (xh + xl);
        xr = 0.5f * (xh - xl);
        M = -__builtin_inff();
#pragma nounroll
        for (int k = 0; k < WMARG_K; ++k) {
            const float l = wiener_marginal_node(b, r, fmaf(xr, wmarg_node(k), xc), t, censored, sd, m);
            buf[k * stride] = l;
            M = fmaxf(M, l);
        }
        M = fmaxf(M, -3.0e38f);
        if (pass < WMARG_PASSES - 1) {
            int first = WMARG_K - 1, last = 0;
            for (int k = 0; k < WMARG_K; ++k) {
                const bool in = buf[k * stride] >= M - WMARG_BAND;
                first = in && k < first ? k : first;
                last = in ? k : last;
            }
            if (first > last) { first = 0; last = WMARG_K - 1; }
            const float nxl = first == 0 ? xl : fmaf(xr, wmarg_node(first - 1), xc);
            const float nxh = last == WMARG_K - 1 ? xh : fmaf(xr, wmarg_node(last + 1), xc);
            xl = nxl; xh = nxh;
        }
    }
    // the value's sum, and the re-walk: W_k = w_k e^{l_k - M} weighs the node's partials; the denominator is the value's own sum
    float nt = 0.0f, na = 0.0f, nw = 0.0f, nv = 0.0f, n1 = 0.0f, n2 = 0.0f;
    sum = 0.0f;
#pragma nounroll
    for (int k = 0; k < WMARG_K; ++k) {
        const float e = __expf(buf[k * stride] - M);
        sum = fmaf(wmarg_weight(k), e, sum);
        const float W = wmarg_weight(k) * e;
        const float x = fmaf(xr, wmarg_node(k), xc);
        int sdk = sd;
        WMGRAD_PER_NODE(sdk);
        const WienerMarginalPartials h = wiener_marginal_node_partials(b, r, g, x, t, censored, sdk);
        const float d = fmaf(__expf(x - r.ldc), r.dc, -m);              // a - m, as the node forms it
        const bool on = W > 0.0f;                                       // (an underflowed node adds nothing: its partials may be infinite)
        nt += on ? W * h.ht : 0.0f;
        na += on ? W * h.xa : 0.0f;
        nw += on ? W * h.hw : 0.0f;
        nv += on ? W * h.hv : 0.0f;
        n1 += on ? W * d : 0.0f;
        n2 += on ? W * (d * d) : 0.0f;
    }
    const float dz = zz - r.gm;
    float out = r.c0 - (dz * dz) * r.i2s + M + logf(sum) + logf(xr);
    if (dead) out = censored ? __builtin_nanf("") : -__builtin_inff();
    if (zbad || y != y) out = __builtin_nanf("");
    s.v += (double)(out * r.valid * b.valid);
    const float id = 1.0f / sum;                                        // (every node at -inf: 0 / 0, a NaN gradient)
    const double e1 = (double)(n1 * id), zd = (double)zz, dzd = zd - gmd;
    s.t += (double)(nt * id);
    s.a += (double)(na * id);
    s.w += (double)(nw * id);
    s.nu += (double)(nv * id);
    s.m1 += e1;
    s.zm += zd * e1;
    s.m2 += (double)(n2 * id);
    s.dz += dzd;
    s.dz2 += dzd * dzd;
    s.poison += (dead || zbad || y != y) ? __builtin_nanf("") : 0.0f;
}

// phi(x) / Phi(x), float64; below 0 from erfcx: sqrt(2 / pi) / erfcx(-x / sqrt 2) keeps its digits where Phi underflows
__device__ __forceinline__ double wiener_marginal_mills(double x)
{
    const double c = 0.797884560802865356, xs = x * 0.707106781186547524;
    return x < 0.0 ? c / erfcx(-xs) : c * exp(-xs * xs) / erfc(-xs);
}

// The row's ten sums -> its log-likelihood and its gradient in the eight parameter columns (float64; lane 0 of the kernel).  n: trials.
__device__ __forceinline__ void wiener_marginal_grad_finish(const float *p, float valid, int n_trials, const WienerMarginalGradAcc &s, double *out_sum,
                                                            double *out_grad)
{
    if (out_sum) *out_sum = s.v;
    const double drift = p[0], mu = p[1], sd = p[4], dc = p[5], s1 = p[6], g = p[7], n = (double)n_trials, nan = (double)valid;
    const double v1 = s1 * s1, va = sd * sd, s2m = v1 + g * g * va, is = 1.0 / s2m;
    const double k0 = mu * v1 * is, k1 = g * va * is, tau2 = va * v1 * is, tau = sqrt(tau2);
    // the integral's share: sum d/dm, sum z d/dm, sum d/dtau
    const double Gm = s.m1 / tau2, Gz = s.zm / tau2, Gt = s.m2 / (tau2 * tau) - n / tau;
    const double mills = wiener_marginal_mills(mu / sd);
    const double idc = 1.0 / dc, vp = drift * idc;
    out_grad[0] = s.nu * idc * nan;
    // m = k0 + k1 z: dm/dmu = v1 / s2m; dm/dsd = 2 sd g (z - g m) / s2m; dm/ds1 = 2 s1 (mu - m) / s2m; dm/dg = va (z - 2 g m) / s2m
    // tau: dtau/dsd = tau v1 / (sd s2m); dtau/ds1 = tau g^2 va / (s1 s2m); dtau/dg = -tau g va / s2m
    out_grad[1] = (Gm * v1 * is + g * s.dz * is - n * mills / sd) * nan;
    out_grad[2] = s.w * nan;
    out_grad[3] = -s.t * nan;
    out_grad[4] = (2.0 * sd * g * is * ((1.0 - g * k1) * Gz - g * k0 * Gm) + Gt * tau * v1 * is / sd
                   + g * g * sd * is * (s.dz2 * is - n) + n * mills * mu / va) * nan;
    out_grad[5] = -(s.a + vp * s.nu) * idc * nan;
    out_grad[6] = (2.0 * s1 * is * ((mu - k0) * Gm - k1 * Gz) + Gt * tau * g * g * va * is / s1 + s1 * is * (s.dz2 * is - n)) * nan;
    out_grad[7] = (va * is * ((1.0 - 2.0 * g * k1) * Gz - 2.0 * g * k0 * Gm) - Gt * tau * g * va * is
                   + g * va * is * (s.dz2 * is - n) + mu * s.dz * is) * nan;
}

// STAGED: the workgroup's rows all score one data set, read from LDS (broadcast layout); else every row reads its own (paired layout)
template <bool STAGED>
__global__ __launch_bounds__(256) void wiener_marginal_grad_kernel(WienerMarginalGradArgs G)
{
    __shared__ float2 tile[STAGED ? WIENER_TILE : 1];
    __shared__ float nodes[WMARG_K * 256];                              // a pass's node values, [k][thread]
    static_assert(WMGRAD_RPW == 1, "a wave holds one row's ten partial sums");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WienerWaveRow w = wiener_wave_row<STAGED, WMGRAD_ROWS>(G.R, G.S, G.chunks, wave);
    if (!STAGED && !w.has_row) return;
    const float *p = G.params + w.row * G.P;
    // every lane works out the row's constants; the wave keeps lane 0's copy as uniform values
    WienerRow b;
    WienerMarginalRow r;
    WienerGradRow g;
    {
        const WienerRow mine = wiener_marginal_base(p);
        const WienerMarginalRow rmine = wiener_marginal_row(p);
        const float pb[5] = {p[0], p[5], p[2], 0.0f, p[5]};
        const WienerGradRow gmine = wiener_grad_row<NDDM_BASIC_DDM_DC>(pb, mine);
        const float *m = reinterpret_cast<const float *>(&mine), *rm = reinterpret_cast<const float *>(&rmine);
        const float *gm = reinterpret_cast<const float *>(&gmine);
        float *bw = reinterpret_cast<float *>(&b), *rw = reinterpret_cast<float *>(&r), *gw = reinterpret_cast<float *>(&g);
#pragma unroll
        for (int f = 0; f < WIENER_ROW_WORDS; ++f) bw[f] = wiener_bcast(m[f], 0);
#pragma unroll
        for (int f = 0; f < WMARG_ROW_WORDS; ++f) rw[f] = wiener_bcast(rm[f], 0);
#pragma unroll
        for (int f = 0; f < WIENER_GRAD_ROW_WORDS; ++f) gw[f] = wiener_bcast(gm[f], 0);
    }
    const double gmd = (double)p[7] * (double)p[1];
    float *buf = nodes + threadIdx.x;
    WienerMarginalGradAcc s = wiener_marginal_grad_zero();
    wiener_row_trials<STAGED, false>(tile, G.data, G.S, G.N, w, lane,
                                     [&](int, float x0, float x1) { wiener_marginal_grad_trial(b, r, g, gmd, x0, x1, G.t_censor, buf, 256, s); });
    if (!w.has_row) return;
    wiener_marginal_grad_reduce(s);
    if (lane == 0) wiener_marginal_grad_finish(p, r.valid * b.valid, G.N, s, G.out_sum ? G.out_sum + w.row : nullptr, G.out_grad + w.row * WMGRAD_COLS);
}

}  // namespace nddm
