// nddm_wiener_quantile.h -- batched Wiener first-passage QUANTILE function (gfx950): the inverse of the distribution function in
// nddm_wiener_cdf.h (RWiener / HDDM qwiener), one independent value per (parameter row, request).  Included by nddm_kernels.hip after
// nddm_wiener_cdf.h, whose row constants (WienerCdfSide), two forms (wiener_cdf_small / wiener_cdf_tail) and conventions it shares; no
// new mathematics.  DESIGN.md section 13.
//
// A request is (p, code).  It names a function G of the decision time t and a target:
//     code > 0: G = F_upper, limit P(upper);   code < 0: G = F_lower, limit P(lower);   code == 0: G = F_lower + F_upper, limit 1
//     flags 0 (defective): target = p;   NDDM_QUANTILE_CONDITIONAL: target = p * limit
// and the kernel writes rt = tau + t with G(t) = target.  The solver works in t alone: tau enters in that last add and nowhere else.
//
// The solver.  G(t*) at the row's switch point t* = WIENER_U_STAR a'^2 is a row constant; it tells which form the root lies in, so a
// request evaluates ONE form throughout: the small-time one on the bracket (0, t*], or the large-time one on [t*, 1e15] (the time at
// which wiener_cdf_tail clamps, where G is its limit exactly).  In each region G is close to a straight line in transformed
// coordinates:
//     small time:  log G     against -1/t, slope r_0^2 / 2 (the leading term's e^{-r_0^2 / (2t)}),
//     large time: -log(P - G) against t,   slope lambda = pi^2 / (2a^2) + (v - a w eta^2)^2 / (2 D(t*)^2) (the k = 1 term's decay),
// so the first step goes from t* along that slope and every later one is the secant through the last two evaluated points in those
// coordinates.  Every step is kept inside the bracket G(lo) < target <= G(hi): a candidate that is not strictly inside it is replaced
// by the midpoint of the bracket's BIT PATTERNS (positive floats order as their integers), and after WQUANT_SECANT_EVALS evaluations
// every step is such a bisection step.  The bracket's width, below 2^31 bit patterns at the start, halves with each of those, so the loop
// ends on adjacent floats after at most WQUANT_SECANT_EVALS + 31 evaluations whatever G does: its trip count is WQUANT_MAX_EVALS, a
// constant, and no exit depends on convergence.  It ends early when |G(t) - target| <= WQUANT_TOL_REL target + WQUANT_TOL_ABS
// (2^-18 and 2^-24), the rounding noise of the float32 G itself (a fifth of the distribution function's 2e-5 bar at most).  The
// accuracy is ABSOLUTE, as the distribution function's is: below a target of about 1e-5 the absolute term dominates, and a target of
// 1e-7 is answered to within 6e-8 of G -- inside the bar, but a relative error of order 1.  Relative accuracy in the far lower tail is
// not promised here either.
//
// Special values, a pure function of (row, p, code): an invalid row (wiener_row's conditions) gives NaN for all its requests, its
// neighbours unaffected; p NaN, p < 0 or code NaN: NaN; p == 0: tau; defective: p > limit NaN, p == limit +inf; conditional: p > 1
// NaN, limit == 0 NaN, p == 1 +inf; a target G does not reach at 1e15 in float32: +inf; alpha_not_scaled's Nu is clipped to +-5.
//
// Execution: the geometry of wiener_cdf_kernel (4 waves own WIENER_ROWS rows; threads 0..31 leave the rows' constants in LDS; the
// broadcast layout stages the request set in LDS one WIENER_TILE at a time, the paired one reads each row's own).  One inlined
// per-request function on both layouts.  No scratch memory, no atomics; stores are plain vector stores.
#pragma once
#include "nddm_wiener_cdf.h"

namespace nddm {

constexpr int WQUANT_SECANT_EVALS = 16;         // evaluations that may be secant steps; every later one bisects
constexpr int WQUANT_MAX_EVALS = WQUANT_SECANT_EVALS + 32;      // the solver's trip count (31 bisections end on adjacent floats)
constexpr float WQUANT_T_MAX = 1.0e15f;         // wiener_cdf_tail's clamp: G is its limit there
constexpr float WQUANT_TOL_REL = 3.814697265625e-06f;           // 2^-18: the solver stops at |G - target| <= TOL_REL target + TOL_ABS
constexpr float WQUANT_TOL_ABS = 5.9604644775390625e-08f;       // 2^-24

struct WienerQuantileArgs {
    const float *params;        // [R, P]
    const float *data;          // [D, N, 2] = (p, boundary code): the requests `probs`, under the name wiener_launch fills
    float *out_q;               // [R, N]
    long long R, S;             // rows, rows per request set
    long long chunks;           // workgroups per request set (broadcast layout)
    int N, P;
    unsigned flags;
};

// The row constants the solver adds to WienerCdfSide, per boundary: P - G at the switch point and the two regions' first slopes
struct WienerQuantileSide {
    float tail_star;            // (P - F)(t*), clamped as wiener_cdf_value clamps it
    float lam;                  // pi^2 / (2 a^2) + (v - a w eta^2)^2 / (2 D(t*)^2)
};

__device__ __forceinline__ WienerQuantileSide wiener_quantile_side(const WienerCdfSide &c)
{
    WienerQuantileSide q;
    q.tail_star = fminf(fmaxf(wiener_cdf_tail(c, c.tstar), 0.0f), c.P);
    const float m = c.mun / (1.0f + c.e2 * c.tstar);
    q.lam = 0.5f * (m * m) - c.lq;
    return q;
}

// G(t) on boundary sd, or on both, by the form of the region the root lies in -- the value wiener_cdf_value gives at rt - tau = t -- and
// the ordinate y the secant works with
__device__ __forceinline__ float wiener_quantile_eval(const WienerCdfSide *cs, int sd, bool both, bool small, float t, float &y)
{
    const float tc = fmaxf(t, 1.17549435e-38f);
    float G = 0.0f, tl = 0.0f;
#pragma nounroll
    for (int s = 0; s < 2; ++s) {
        if (!both && s != sd) continue;
        const WienerCdfSide &c = cs[s];
        if (small) {
            G += fminf(fmaxf(wiener_cdf_small(c, tc), 0.0f), c.P);
        } else {
            const float x = fminf(fmaxf(wiener_cdf_tail(c, tc), 0.0f), c.P);
            tl += x;
            G += c.P - x;
        }
    }
    y = small ? __logf(G) : -__logf(tl);
    return G;
}

// rt of one request: a pure function of (row constants, p, code, flags).  evals: the number of evaluations of G it took -- read by
// tools/wiener_quantile_host.py (this code compiled for the host) alone; the kernel drops it, and it is no device output.
__device__ __forceinline__ float wiener_quantile_request(const WienerCdfSide *cs, const WienerQuantileSide *qs, float p, float code,
                                                         unsigned flags, int &evals)
{
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    evals = 0;
    const bool both = code == 0.0f;
    const int sd = code > 0.0f ? 1 : 0;
    const float tau = cs[0].tau, tstar = cs[0].tstar;
    if (!(cs[0].valid == cs[0].valid) || !(p >= 0.0f) || !(code == code)) return nan;
    if (p == 0.0f) return tau;
    const float P = both ? 1.0f : cs[sd].P;                             // the limit of G
    float T;
    if (flags & NDDM_QUANTILE_CONDITIONAL) {
        if (!(p <= 1.0f) || !(P > 0.0f)) return nan;
        if (p == 1.0f) return inf;
        T = p * P;
    } else {
        if (!(p <= P)) return nan;
        if (p == P) return inf;
        T = p;
    }
    if (!(T > 0.0f)) return tau;                                        // (p P below the smallest float)
    // what G gives at the two ends of the large-time bracket, in float32
    const float Pd = both ? cs[0].P + cs[1].P : P;
    if (!(Pd >= T)) return inf;
    const float ts = both ? qs[0].tail_star + qs[1].tail_star : qs[sd].tail_star;
    const float Fs = both ? (cs[0].P - qs[0].tail_star) + (cs[1].P - qs[1].tail_star) : P - ts;
    const float tol = WQUANT_TOL_REL * T + WQUANT_TOL_ABS;
    if (fabsf(Fs - T) <= tol) return tau + tstar;
    const bool small = T < Fs;
    float lo = small ? 0.0f : tstar, hi = small ? tstar : WQUANT_T_MAX;   // G(lo) < T <= G(hi)
    // the last evaluated point in the region's coordinates, and the candidate the model's slope gives from it
    float x1 = small ? -1.0f / tstar : tstar;
    float y1 = small ? __logf(Fs) : -__logf(ts);
    const float yT = small ? __logf(T) : -__logf(Pd - T);
    const float m = small ? (both ? fminf(cs[0].hr2[0], cs[1].hr2[0]) : cs[sd].hr2[0]) : (both ? fminf(qs[0].lam, qs[1].lam) : qs[sd].lam);
    float xc = x1 + (yT - y1) / m;
#pragma nounroll
    for (int it = 0; it < WQUANT_MAX_EVALS; ++it) {
        const unsigned lb = __float_as_uint(lo), hb = __float_as_uint(hi);
        if (hb - lb <= 1u) break;
        const float tc = small ? -1.0f / xc : xc;
        const bool ok = it < WQUANT_SECANT_EVALS && tc > lo && tc < hi;  // (a NaN candidate fails both)
        const float t = ok ? tc : __uint_as_float(lb + ((hb - lb) >> 1));
        float y;
        const float G = wiener_quantile_eval(cs, sd, both, small, t, y);
        ++evals;
        if (fabsf(G - T) <= tol) { hi = t; break; }
        if (G < T) lo = t; else hi = t;
        const float x = small ? -1.0f / t : t;
        xc = x + (yT - y) * ((x - x1) / (y - y1));
        x1 = x; y1 = y;
    }
    return tau + hi;
}

// STAGED: the workgroup's rows all answer one request set, staged in LDS (broadcast layout); else every row reads its own (paired layout)
template <int MODEL, bool STAGED>
__global__ __launch_bounds__(256) void wiener_quantile_kernel(WienerQuantileArgs A)
{
    __shared__ float2 tile[STAGED ? WIENER_TILE : 1];
    __shared__ WienerCdfSide sides[WIENER_ROWS][2];
    __shared__ WienerQuantileSide qsides[WIENER_ROWS][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long rbase, rend;
    wiener_block_rows<STAGED, WIENER_ROWS>(A.R, A.S, A.chunks, rbase, rend);
    // thread 2k + side works out the constants of row k on that boundary (rows past the end repeat the last one and are never read)
    if (threadIdx.x < 2 * WIENER_ROWS) {
        const int lr = threadIdx.x >> 1, side = threadIdx.x & 1;
        const long long r = rbase + lr < rend ? rbase + lr : rend - 1;
        const float *p = A.params + r * A.P;
        const WienerRow wr = wiener_row<MODEL>(p);
        const WienerCdfSide c = wiener_cdf_side<MODEL>(wr, p, side);
        sides[lr][side] = c;
        qsides[lr][side] = wiener_quantile_side(c);
    }
    __syncthreads();
    const long long wrow0 = rbase + wave;                               // the wave's rows: wrow0 + 4k, k < WIENER_RPW
    for (int t0 = 0; t0 < A.N; t0 += WIENER_TILE) {
        const int nt = wiener_enter_tile<STAGED>(tile, A.data, A.S, A.N, rbase, t0);       // (staged once for the wave's four rows)
#pragma nounroll
        for (int k = 0; k < WIENER_RPW; ++k) {
            const long long row = wrow0 + 4ll * k;
            if (row >= rend) break;                                     // wave-uniform
            const int lr = wave + 4 * k;
            float *dst = A.out_q + row * (long long)A.N + t0;
            wiener_tile_trials<STAGED, false>(tile, A.data, A.S, A.N, row, t0, nt, lane, [&](int i, float x0, float x1) {
                int evals;
                dst[i] = wiener_quantile_request(sides[lr], qsides[lr], x0, x1, A.flags, evals);
            });
        }
    }
}

}  // namespace nddm
