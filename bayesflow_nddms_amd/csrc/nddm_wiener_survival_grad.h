// nddm_wiener_survival_grad.h -- log S = log P(T > t) of the eta = 0 process and its partials in (a', w = beta, v') at fixed t (gfx950): what a
// censored timeout contributes to a gradient.  ONE function of (WienerRow, t), wiener_log_survival_grad, in both of wiener_log_survival's
// forms and with its select.  Included by nddm_wiener_grad.h (basic_ddm_dc's censored rows, DESIGN.md section 14, which adds d/dt) and through
// it by nddm_wiener_marginal_grad.h (the single-trial model's timeouts, section 16, where t_censor is a constant of the call).
//     images (u < WIENER_SURV_U): every one of the twelve terms is 1/2 e^{G} erfc(z), G = v' d, z linear in (a' w + t v' + d) / sqrt(2t);
//       its partial is G_theta term - pi^-1/2 e^{G - z^2} z_theta: the same erfcx scaling, plus the exponential e^{G - z^2} itself.  The
//       common e^{sigma} is a constant of the trial and cancels in the ratio of sums.
//     series (u >= WIENER_SURV_U): S = (pi / a'^2) sum_k k sin(k pi w) e^{-lambda_k t} / lambda_k (e^{-a' v' w} + (-1)^{k+1} e^{a' v' (1 - w)});
//       each term is differentiated in a', w, v' (d/da' lambda_k = -k^2 pi^2 / a'^3, d/dv' lambda_k = v'; cos(k pi w) by the same Chebyshev
//       recurrence as sin(k pi w)) and the ratio of sums taken, with the same stopping rule on the same `env`; the factors common to
//       every term (1 / a'^2, and e^{-a' v' w} in w) are differentiated in closed form.
#pragma once
#include "nddm_wiener.h"

namespace nddm {

// log S = log P(T > t) of the eta = 0 process and its partials in (a', w = beta, v') at fixed t
struct WienerSurvivalGrad {
    float ls, da, dw, dv;
};

// The images (wiener_log_survival_small's twelve trips, its scaling and its value): contribution s_i s_f T, T = 1/2 e^{G} erfc(z), s_i the
// image's sign and s_f = -1 for the far (q) term; z = s_f D with D the drifted centre's distance beyond a (dU) or below 0 (dL), so its
// partial is G_theta (s_f T) - E D_theta with E = pi^-1/2 e^{G - z^2}, whichever the sign of z.
__device__ __forceinline__ WienerSurvivalGrad wiener_log_survival_grad_small(const WienerRow &row, float t)
{
    const float ap = row.ap, vp = row.vp, w0 = row.w[0], w1 = row.w[1];
    t = fmaxf(t, 1.0e-30f);
    float rs = __builtin_amdgcn_rsqf(2.0f * t);
    rs = rs * fmaf(-t * rs, rs, 1.5f);
    const float x0 = ap * w0, a2 = 2.0f * ap;
    const float mL = fmaf(t, vp, x0);
    const float mU = fmaf(t, vp, -(ap * w1));
    const float p0 = fmaxf(mU, -mL) * rs;
    const float sigma = p0 > 0.0f ? p0 * p0 : 0.0f;
    float acc = 0.0f, na = 0.0f, nw = 0.0f, nv = 0.0f;
#pragma nounroll
    for (int k = 0; k < 12; ++k) {
        const int i = k >> 1;
        const bool neg = i & 1, far = k & 1;
        const float n2 = 2.0f * (float)((i >> 1) - 1);                  // 2n: the image sits at +-x0 + 2 n a'
        const float d = (float)((i >> 1) - 1) * a2 - (neg ? 2.0f * x0 : 0.0f);
        const float G = fmaf(vp, d, sigma), dU = (mU + d) * rs, dL = -(mL + d) * rs;
        const bool up = dU > dL;
        const float p = fmaxf(dU, dL), z = far ? -fminf(dU, dL) : p;
        const float h = wiener_half_exp_erfcx(fmaf(-z, z, G), fabsf(z));
        const float term = far ? -h : (p >= 0.0f ? h : __expf(fminf(G, 80.0f)) - h);
        const float E = 0.564189583547756287f * __expf(fminf(fmaf(-z, z, G), 80.0f));
        // the centre x0 + d + t v' = a' cw + t v', cw = +-w + 2n; d = a' dw
        const float cw = neg ? n2 - w0 : n2 + w0, dw = neg ? n2 - 2.0f * w0 : n2;
        const bool useU = up != far;                                    // D = dU (the centre minus a') or dL (minus the centre)
        const float sD = useU ? rs : -rs;
        const float Da = useU ? (cw - 1.0f) * rs : -cw * rs;
        const float Dw = (neg ? -ap : ap) * sD;
        const float Dv = t * sD;
        const float ca = fmaf(vp * dw, term, -E * Da);
        const float cwv = fmaf(neg ? -a2 * vp : 0.0f, term, -E * Dw);
        const float cv = fmaf(d, term, -E * Dv);
        acc = neg ? acc - term : acc + term;
        na = neg ? na - ca : na + ca;
        nw = neg ? nw - cwv : nw + cwv;
        nv = neg ? nv - cv : nv + cv;
    }
    const float sacc = fmaxf(acc, 1.17549435e-38f);
    const float ia = 1.0f / sacc;
    WienerSurvivalGrad g;
    g.ls = fminf(0.693147180559945309f * __builtin_amdgcn_logf(sacc) - sigma, 0.0f);
    g.da = na * ia; g.dw = nw * ia; g.dv = nv * ia;
    return g;
}

// The series (wiener_log_survival_large's terms, its stopping rule and its value), each term differentiated
__device__ __forceinline__ WienerSurvivalGrad wiener_log_survival_grad_large(const WienerRow &c, float t)
{
    const float m = fmaxf(c.d0[0], c.d0[1]);
    const float wl = __expf(c.d0[0] - m), wu = __expf(c.d0[1] - m);
    const float kk = -c.lq;                                             // pi^2 / (2 a'^2)
    const float lam1 = c.hn2 + kk;
    const float ap = c.ap, vp = c.vp, ia = 1.0f / ap;
    const float bl = -c.w[0] * wl, bu = c.w[1] * wu;                    // d/d(a' v') of the two side weights
    float sk_1 = 0.0f, sk = c.s1, ck_1 = 1.0f, ck = c.cpb, sum = 0.0f, na = 0.0f, nw = 0.0f, nv = 0.0f;
    for (int k = 1; k <= WIENER_SURV_TERMS; ++k) {
        const float fk = (float)k, k2 = fk * fk;
        const float lam = c.hn2 + kk * k2;
        const float sgn = (k & 1) ? 1.0f : -1.0f;
        const float il = __builtin_amdgcn_rcpf(lam);
        const float env = fk * __expf(-kk * (k2 - 1.0f) * t) * il;
        if (k > 1 && env * (wl + wu) < 5.9604644775390625e-08f * fabsf(sum)) break;
        sum += env * (wl * sk + wu * sgn * sk);
        const float B = wl + sgn * wu, dB = bl + sgn * bu, tl = t + il;
        const float es = env * sk;
        na += es * fmaf(B * (2.0f * kk * k2 * ia), tl, vp * dB);      // d/da' lambda_k = -2 kk k^2 / a'
        nv += es * fmaf(-B * vp, tl, ap * dB);                          // d/dv' lambda_k = v'
        nw += env * B * (fk * ck);                                      // d/dw sin(k pi w) = k pi cos(k pi w)
        const float sn = 2.0f * c.cpb * sk - sk_1, cn = 2.0f * c.cpb * ck - ck_1;
        sk_1 = sk; sk = sn;
        ck_1 = ck; ck = cn;
    }
    const float is = 1.0f / sum;
    WienerSurvivalGrad g;
    g.ls = -lam1 * t + m + (1.14472988584940017f - 2.0f * c.la) + 0.693147180559945309f * __builtin_amdgcn_logf(sum);
    g.da = fmaf(na, is, -2.0f * ia);
    g.dw = fmaf(3.14159265358979324f * nw, is, -ap * vp);
    g.dv = nv * is;
    return g;
}

// wiener_log_survival's value and select; t <= 0 is log 1 = 0 with zero partials
__device__ __forceinline__ WienerSurvivalGrad wiener_log_survival_grad(const WienerRow &c, float t)
{
    if (!(t > 0.0f)) {
        const float v = t == t ? 0.0f : t;
        return WienerSurvivalGrad{v, v, v, v};
    }
    return t < (WIENER_SURV_U / WIENER_U_STAR) * c.tstar ? wiener_log_survival_grad_small(c, t) : wiener_log_survival_grad_large(c, t);
}

}  // namespace nddm
