// nddm_wiener_cdf.h -- batched Wiener first-passage DISTRIBUTION function (gfx950): P(T <= t, boundary) and P(upper), the companion of the
// density in nddm_wiener.h (RWiener / HDDM pwiener), one independent value per (parameter row, trial).  Included by nddm_kernels.hip after
// nddm_wiener.h, whose conventions, row constants (WienerRow / wiener_row) and survival series it shares.  DESIGN.md section 12.
//
// Lower boundary with (v', w = beta), upper boundary the same formula with (-v', 1 - beta); a = a', v, eta scaled by s; t = rt - tau,
// D = 1 + eta^2 t, d(t) = (eta^2 a^2 w^2 - 2 a v w - v^2 t) / (2 D) (the density's drift exponent), r_j = a (j + w) for even j and
// a (j + 1 - w) for odd j.  Two FIXED-TRIP forms, switching at the density's WIENER_U_STAR:
//   small time (Gondan, Blurton & Kesselmeier 2014; drift variability integrated in closed form, Blurton et al. 2017), j <= WCDF_SMALL_J:
//     F = 1/2 sum_j (-1)^j [T(c = aw + r_j, +) + T(c = aw - r_j, -)],
//     T(c, +-) = e^{d - r^2/(2t)} erfcx(x),  x = (r -+ t (v - c eta^2)) / sqrt(2 t D)       (x >= 0)
//              = 2 e^{-c v + c^2 eta^2 / 2} - e^{d - r^2/(2t)} erfcx(-x)                    (x < 0; the exponent is <= 0 there)
//     Every factor is an exponential times a scaled erfc, so nothing overflows; e^{d - r^2/(2t)} (which can be large against a tiny
//     erfcx when eta a is large) is applied as two factors e^{(d - r^2/(2t))/2}.  No quadrature at any eta.
//   large time, k <= WCDF_LARGE_K:
//     F = P - (2 pi / a^2) D^{-1/2} e^{d} sum_k k sin(k pi w) e^{-k^2 pi^2 t / (2 a^2)} E_{v ~ N(mu_t, s_t^2)} [1 / (v^2 + k^2 pi^2 / a^2)],
//     mu_t = (v - a w eta^2) / D, s_t = eta / sqrt(D): the prior N(v, eta^2) times e^{-v a w - v^2 t / 2} is that Gaussian times D^{-1/2} e^{d}.
//     The expectation is a WCDF_NODES-point Gauss-Hermite rule on mu_t + s_t z_i (eta = 0: the one point v).  s_t <= 1 / sqrt(t) is at most
//     0.52 of the distance pi / a of the integrand's poles from the real axis at u >= WIENER_U_STAR, where 16 nodes are exact to 8e-8
//     (a rule on the prior itself, up to 2.4 pole distances wide, is off by 1e-3 at 48 nodes and 1e-4 at 96: DESIGN section 12).
//   P = P(boundary): closed form at eta = 0; with eta > 0 it has none and is small(t*) + [P - large](t*) at the switch point t*, once per row.
// Measured in float64 over the accuracy test's domain (tests/test_wiener_cdf_host.py): |scheme - yardstick| <= 8e-8.
//
// Special values follow the density's: t <= 0 gives 0; an invalid row (wiener_row's conditions) gives NaN for its trials and its P(upper),
// its neighbours unaffected; basic_ddm_dc choice 0 (a timeout) gives P(T <= t) over both boundaries, 1 - S(t) of wiener_log_survival;
// alpha_not_scaled y == 0 gives NaN; Nu is clipped to +-5.  The result is clamped into [0, P].
//
// Execution: the geometry of wiener_kernel (4 waves own WIENER_ROWS rows; broadcast layout with the data set staged in LDS, or paired).
// Threads 0..31 work out the constants of the workgroup's 16 rows x 2 boundaries once and leave them in LDS (5 KB); every trial reads
// its row's and boundary's from there.  One inlined per-trial function on both layouts: a value depends on (row, trial) alone.  No
// scratch memory, no atomics; stores are plain vector stores.
#pragma once
#include "nddm_wiener.h"

namespace nddm {

constexpr int WCDF_SMALL_J = 3;                 // j = 0..3 of the small-time series
constexpr int WCDF_LARGE_K = 4;                 // k = 1..4 of the large-time series
constexpr int WCDF_NODES = 16;                  // Gauss-Hermite nodes of the large-time expectation (8 symmetric pairs)

struct WienerCdfArgs {
    const float *params;        // [R, P]
    const float *data;          // [D, N, 2] (NULL when out_cdf is)
    float *out_cdf;             // [R, N] or NULL
    float *out_p_upper;         // [R] or NULL
    long long R, S;             // rows, rows per data set
    long long chunks;           // workgroups per data set (broadcast layout)
    int N, P;
};

// The constants of one row on one boundary (v and w are that boundary's: (v', beta) or (-v', 1 - beta))
struct WienerCdfSide {
    float tau, tstar, valid;    // as WienerRow's
    float v, eta, e2, hn2;      // drift, eta', eta'^2, v^2 / 2
    float d0, mun;              // eta^2 a^2 w^2 / 2 - a v w;  v - a w eta^2
    float lq, lam2;             // -pi^2 / (2 a^2);  pi^2 / a^2
    float P;                    // P(this boundary), eta integrated
    float sk[WCDF_LARGE_K];     // (2 pi / a^2) k sin(k pi w)
    float r[WCDF_SMALL_J + 1], hr2[WCDF_SMALL_J + 1];          // r_j;  r_j^2 / 2
    float pa[WCDF_SMALL_J + 1], pb[WCDF_SMALL_J + 1];          // v - c eta^2 for c = aw + r_j and c = aw - r_j
    float fa[WCDF_SMALL_J + 1], fb[WCDF_SMALL_J + 1];          // 2 e^{-c v + c^2 eta^2 / 2} for the two (inf where never selected)
};

// 1/2 sum_j (-1)^j [T_A + T_B], t > 0 (clamped to the smallest normal float by the caller)
__device__ __forceinline__ float wiener_cdf_small(const WienerCdfSide &c, float t)
{
    const float D = 1.0f + c.e2 * t;
    const float d = (c.d0 - c.hn2 * t) * __builtin_amdgcn_rcpf(D);
    const float it = __builtin_amdgcn_rcpf(t);
    const float rs = __builtin_amdgcn_rsqf(2.0f * t * D);
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j <= WCDF_SMALL_J; ++j) {
        const float eg = __expf(0.5f * (d - c.hr2[j] * it));
        const float xa = (c.r[j] - t * c.pa[j]) * rs, xb = (c.r[j] + t * c.pb[j]) * rs;
        const float ta = eg * (eg * erfcxf(fabsf(xa))), tb = eg * (eg * erfcxf(fabsf(xb)));
        const float term = (xa < 0.0f ? c.fa[j] - ta : ta) + (xb < 0.0f ? c.fb[j] - tb : tb);
        sum = (j & 1) ? sum - term : sum + term;
    }
    return 0.5f * sum;
}

// P - F(t) = P(T > t, this boundary): the large-time series, t > 0
__device__ __forceinline__ float wiener_cdf_tail(const WienerCdfSide &c, float t)
{
    t = fminf(t, 1.0e15f);                                              // (D stays finite; the series is 0 long before)
    const float D = 1.0f + c.e2 * t;
    const float iD = __builtin_amdgcn_rcpf(D), rD = __builtin_amdgcn_rsqf(D);
    const float C = rD * __expf((c.d0 - c.hn2 * t) * iD);
    const float q = __expf(c.lq * t);
    const float q2 = q * q, q4 = q2 * q2, q8 = q4 * q4, q9 = q8 * q, q16 = q8 * q8;
    const float l1 = c.lam2, l2 = 4.0f * c.lam2, l3 = 9.0f * c.lam2, l4 = 16.0f * c.lam2;
    static_assert(WCDF_LARGE_K == 4 && WCDF_NODES == 16, "four series terms, eight node pairs");
    float e1, e2, e3, e4;                                               // E[1 / (v^2 + k^2 pi^2 / a^2)]
    if (c.e2 > 0.0f) {                                                  // row-uniform
        // Gauss-Hermite nodes and weights of N(0, 1), the positive half (the rule is symmetric)
        constexpr float Z[8] = {3.867606045e-01f, 1.163829101e+00f, 1.951980346e+00f, 2.760245048e+00f,
                                3.600873624e+00f, 4.492955303e+00f, 5.472225706e+00f, 6.630878198e+00f};
        constexpr float Wt[8] = {2.865685212e-01f, 1.583383728e-01f, 4.728475235e-02f, 7.266937601e-03f,
                                 5.259849266e-04f, 1.530003216e-05f, 1.309473216e-07f, 1.497814723e-10f};
        const float mu = c.mun * iD, sg = c.eta * rD;
        e1 = e2 = e3 = e4 = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float va = mu + sg * Z[i], vb = mu - sg * Z[i];
            const float a2 = va * va, b2 = vb * vb;
            e1 = fmaf(Wt[i], __builtin_amdgcn_rcpf(a2 + l1) + __builtin_amdgcn_rcpf(b2 + l1), e1);
            e2 = fmaf(Wt[i], __builtin_amdgcn_rcpf(a2 + l2) + __builtin_amdgcn_rcpf(b2 + l2), e2);
            e3 = fmaf(Wt[i], __builtin_amdgcn_rcpf(a2 + l3) + __builtin_amdgcn_rcpf(b2 + l3), e3);
            e4 = fmaf(Wt[i], __builtin_amdgcn_rcpf(a2 + l4) + __builtin_amdgcn_rcpf(b2 + l4), e4);
        }
    } else {
        const float v2 = 2.0f * c.hn2;
        e1 = __builtin_amdgcn_rcpf(v2 + l1); e2 = __builtin_amdgcn_rcpf(v2 + l2);
        e3 = __builtin_amdgcn_rcpf(v2 + l3); e4 = __builtin_amdgcn_rcpf(v2 + l4);
    }
    return C * (c.sk[0] * q * e1 + c.sk[1] * q4 * e2 + c.sk[2] * q9 * e3 + c.sk[3] * q16 * e4);
}

// P(lower boundary) at eta = 0, (1 - e^{-2va(1-w)}) / (e^{2vaw} - e^{-2va(1-w)}) with the exponents kept negative; 1 - w at v = 0
__device__ __forceinline__ float wiener_cdf_p0(float a, float v, float w)
{
    const float m = 2.0f * fabsf(v) * a;
    if (!(m >= 1.0e-6f)) return m == m ? 1.0f - w : m;
    const float r = expm1f(-m * (1.0f - w)) / expm1f(-m);
    return v > 0.0f ? expf(-m * w) * r : r;
}

template <int MODEL>
__device__ __forceinline__ WienerCdfSide wiener_cdf_side(const WienerRow &wr, const float *p, int side)
{
    float v, a, eta, s;                                                 // as wiener_row reads them
    if (MODEL == NDDM_BASIC_DDM_DC) { v = p[0]; a = p[1]; s = p[4]; eta = 0.0f; }
    else { v = p[0]; a = p[1]; eta = p[4]; s = p[5]; }
    if (MODEL == NDDM_ALPHA_NOT_SCALED && (v < -5.0f || v > 5.0f)) v = v > 0.0f ? 5.0f : -5.0f;
    const float ap = a / s, vp = v / s, ep = eta / s;
    WienerCdfSide c;
    c.tau = wr.tau; c.tstar = wr.tstar; c.valid = wr.valid;
    c.v = side ? -vp : vp;
    c.eta = ep; c.e2 = wr.e2; c.hn2 = wr.hn2;
    c.d0 = side ? wr.d0[1] : wr.d0[0];                                  // (selects: a dynamic index would put wr in scratch)
    const float w = side ? wr.w[1] : wr.w[0], aw = ap * w;
    c.mun = c.v - aw * c.e2;
    c.lq = wr.lq;
    c.lam2 = 9.86960440108935862f / (ap * ap);
    const float pref = 6.28318530717958648f / (ap * ap);
#pragma unroll
    for (int k = 1; k <= WCDF_LARGE_K; ++k) c.sk[k - 1] = pref * ((float)k * sinpif((float)k * w));
#pragma unroll
    for (int j = 0; j <= WCDF_SMALL_J; ++j) {
        const float r = (j & 1) ? ap * ((float)(j + 1) - w) : ap * ((float)j + w);
        const float ca = aw + r, cb = aw - r;
        c.r[j] = r;
        c.hr2[j] = 0.5f * (r * r);
        c.pa[j] = c.v - ca * c.e2;
        c.pb[j] = c.v - cb * c.e2;
        c.fa[j] = 2.0f * expf(0.5f * (ca * ca) * c.e2 - ca * c.v);
        c.fb[j] = 2.0f * expf(0.5f * (cb * cb) * c.e2 - cb * c.v);
    }
    c.P = 0.0f;
    if (c.e2 > 0.0f) c.P = wiener_cdf_small(c, c.tstar) + wiener_cdf_tail(c, c.tstar);
    else c.P = wiener_cdf_p0(ap, c.v, w);
    c.P = fminf(fmaxf(c.P, 0.0f), 1.0f) * c.valid;
    return c;
}

// P(T <= rt - tau, this boundary): a pure function of (row constants, rt)
__device__ __forceinline__ float wiener_cdf_value(const WienerCdfSide &c, float rt)
{
    const float t = rt - c.tau;
    const float tc = fmaxf(t, 1.17549435e-38f);
    const float F = t < c.tstar ? wiener_cdf_small(c, tc) : c.P - wiener_cdf_tail(c, tc);
    return (t > 0.0f ? fminf(fmaxf(F, 0.0f), c.P) : 0.0f) * c.valid;      // (c.P is NaN on an invalid row, as valid is)
}

template <int MODEL>
__device__ __forceinline__ float wiener_cdf_trial(const WienerCdfSide *sides, const WienerRow *wr, float x0, float x1)
{
    if (MODEL == NDDM_BASIC_DDM_DC) {                                   // (rt, choice): 1 upper, -1 lower, 0 a timeout -> P(T <= t)
        if (x1 == 0.0f) {
            const float t = x0 - sides[0].tau;
            return (t > 0.0f ? fminf(fmaxf(1.0f - __expf(wiener_log_survival(*wr, t)), 0.0f), 1.0f) : (t == t ? 0.0f : t)) * sides[0].valid;
        }
        return wiener_cdf_value(sides[x1 > 0.0f ? 1 : 0], x0) + (x1 == x1 ? 0.0f : x1);
    } else {                                                            // (y, acc): rt = |y|, upper iff y > 0; y == 0 has no time
        const float r = wiener_cdf_value(sides[x0 > 0.0f ? 1 : 0], fabsf(x0));
        return x0 == 0.0f ? __builtin_nanf("") : r;
    }
}

// STAGED: the workgroup's rows all read one data set, staged in LDS (broadcast layout); else every row reads its own (paired layout)
template <int MODEL, bool STAGED>
__global__ __launch_bounds__(256) void wiener_cdf_kernel(WienerCdfArgs A)
{
    __shared__ float2 tile[STAGED ? WIENER_TILE : 1];
    __shared__ WienerCdfSide sides[WIENER_ROWS][2];
    __shared__ WienerRow wrows[MODEL == NDDM_BASIC_DDM_DC ? WIENER_ROWS : 1];     // (the timeouts' survival series)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long rb, re;
    wiener_block_rows<STAGED, WIENER_ROWS>(A.R, A.S, A.chunks, rb, re);
    const long long rbase = rb, rend = re;                              // (constants from here on: the p_upper guard below compiles to one scalar instruction more otherwise)
    // thread 2k + side works out the constants of row k on that boundary (rows past the end repeat the last one and are never read)
    if (threadIdx.x < 2 * WIENER_ROWS) {
        const int lr = threadIdx.x >> 1, side = threadIdx.x & 1;
        const long long r = rbase + lr < rend ? rbase + lr : rend - 1;
        const float *p = A.params + r * A.P;
        const WienerRow wr = wiener_row<MODEL>(p);
        const WienerCdfSide c = wiener_cdf_side<MODEL>(wr, p, side);
        sides[lr][side] = c;
        if (MODEL == NDDM_BASIC_DDM_DC && side == 0) wrows[lr] = wr;
        if (A.out_p_upper && side == 1 && rbase + lr < rend) A.out_p_upper[r] = c.P;
    }
    __syncthreads();
    if (!A.out_cdf) return;
    const long long wrow0 = rbase + wave;                               // the wave's rows: wrow0 + 4k, k < WIENER_RPW
    for (int t0 = 0; t0 < A.N; t0 += WIENER_TILE) {
        const int nt = wiener_enter_tile<STAGED>(tile, A.data, A.S, A.N, rbase, t0);       // (staged once for the wave's four rows)
#pragma nounroll
        for (int k = 0; k < WIENER_RPW; ++k) {
            const long long row = wrow0 + 4ll * k;
            if (row >= rend) break;                                     // wave-uniform
            const int lr = wave + 4 * k;
            const WienerCdfSide *cs = sides[lr];
            const WienerRow *wr = &wrows[MODEL == NDDM_BASIC_DDM_DC ? lr : 0];
            float *dst = A.out_cdf + row * (long long)A.N + t0;
            wiener_tile_trials<STAGED, false>(tile, A.data, A.S, A.N, row, t0, nt, lane,
                                              [&](int i, float x0, float x1) { dst[i] = wiener_cdf_trial<MODEL>(cs, wr, x0, x1); });
        }
    }
}

}  // namespace nddm
