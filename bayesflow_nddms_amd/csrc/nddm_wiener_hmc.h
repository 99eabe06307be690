// nddm_wiener_hmc.h -- batched Hamiltonian Monte Carlo over the basic_ddm_dc Wiener posterior (gfx950): the reference's likelihood-based
// fit (basic_ddm_dc_pyjags.py:103-137: 100 participants x 6 chains x 12 000 iterations of JAGS over dwiener) as independent chains, ONE
// WAVE PER CHAIN, persistent through all the iterations of a launch.  A chain is sequential; a fit is hundreds of chains that share
// nothing, and each gradient is a reduction over the chain's trials: data-parallel the way the simulator is.  Included by
// nddm_kernels.hip (one translation unit) after nddm_wiener_grad.h, whose wiener_row / wiener_grad_row / wiener_grad_trial /
// wiener_grad_finish give the likelihood and its gradient -- called, not copied.  DESIGN.md section 17.
//
// Posterior, in this project's column order (drift, boundary, beta, tau, dc):
//     drift    ~ N(0, 2^2)          all of R
//     boundary ~ N(1, .5^2)         (0, 10)
//     beta     ~ Beta(2, 2)         (0, 1)
//     tau      ~ N(.5, .25^2)       (0, T),  T = min(1.5, the smallest response time of the data set)
//     dc       ~ N(1, .5^2)         (WHMC_DC_MIN, 10)
// The dc floor is a deviation from the JAGS model (support (0, 10)): it keeps the chain inside the domain the Wiener kernels are tested on.
// The truncation constants of the priors are dropped, and tau's upper limit is the data's and not the prior's 1.5 where the data are
// tighter (beyond min rt the likelihood is zero): the log posterior is defined UP TO AN ADDITIVE CONSTANT.
//
// Coordinates: q in R^5 unconstrained, drift = q0, a bounded column theta = lo + (hi - lo) sigma(q).  The log posterior in q adds the
// log-Jacobian sum [log(hi - lo) + log sigma + log(1 - sigma)]; its gradient is (dloglik/dtheta + dlogprior/dtheta) (hi - lo) sigma (1 - sigma)
// + (1 - 2 sigma).  All of the chain's scalar arithmetic (q, momentum, Hamiltonian, transforms, adaptation) is float64; theta is cast to
// float32 for the likelihood.  A column whose free_mask bit is clear is FIXED: its slot of q holds theta itself and never changes, its
// momentum and gradient are zero, its prior and Jacobian terms are left out.
//
// Iteration g of chain c: momentum p_j = z_j / sqrt(inv_mass_j); step eps (0.8 + 0.2 u1); n_leapfrog leapfrog steps; accept when
// log u2 < H0 - H1.  A non-finite H1 or H1 - H0 > 1000 is a rejection counted as divergent.  The first n_adapt iterations of a chain
// adapt log eps by dual averaging (Hoffman & Gelman 2014, algorithm 5: delta .8, gamma .05, t0 10, kappa .75, mu from the state); after the
// last of them eps = eps-bar.  Randomness: two Philox4x32-10 blocks per iteration, key = seed, counter (global chain index, global
// iteration index, WHMC_TAG | block, WHMC_TAG) -- no simulator stream has that tag in either word -- giving five normals by the EXACT
// Box-Muller of nddm_rng.h (a host build draws the same bits) and the two uniforms.  A chain's output is a pure function of (seed, global
// chain index, its data set, its incoming state, inv_mass, free_mask, n_leapfrog, thin, n_adapt, the iteration range): not of the grid,
// the other chains of the launch, or how the range is cut into launches.
//
// State, double [C, WHMC_STATE]: q[5], log eps, log eps-bar, H-bar, mu, adapting iterations done, and two words the chain only reports in:
// the last iteration's energy error H1 - H0, and the largest finite |H1 - H0| so far (what the energy tests read; a NaN coming in is ignored).
//
// Execution: 256 threads = 4 waves = 4 chains per workgroup, chain c on data set c / chains_per_dataset.  Lane j stages trials j, j + 64, ...
// of the wave's data set in the wave's own WHMC_MAX_TRIALS pairs of LDS and reads back only those: no barrier and no exchange between or
// inside waves after it.  While staging the wave finds T and whether the data set can be sampled at all.  Per gradient, lane j accumulates
// its trials in float64 in wiener_grad_kernel's order, the butterfly leaves every lane with the six sums, and every lane does the chain
// rule and the leapfrog update redundantly (the values are wave-uniform, so is every branch).  Lane 0 stores the kept draws.  No scratch
// memory, no atomics; stores are plain vector stores.
//
// A chain is FLAGGED -- no iteration, NaN draws, flagged = 1, state unchanged, neighbours unaffected -- when its data set holds a
// choice-0 trial (without NDDM_WIENER_CENSORED), a non-finite value or a response time <= 0, or when its incoming state is not finite.
// All of it is found by reading values.
//
// NDDM_WIENER_CENSORED (the CENSORED template argument, from the kernel's body down to wiener_grad_trial): choice 0 is a trial, scored
// right-censored by nddm_wiener_grad.h's censored instantiation in the same sweep, and T is the smallest rt of the RESPONSES (1.5 when the
// data set has none).  The streams, the state, the bounds and the purity statement are unchanged; with no timeout in the data the bits
// are the unflagged chain's.  wiener_hmc_kernel holds none of the survival code; wiener_hmc_censored_kernel is a kernel of its own.
//
// WHMC_HOST: the host build (tools/wiener_hmc_host.py) compiles everything but the kernel against a stand-in for <hip/hip_runtime.h>, the
// 64 lanes as a loop and the butterfly in the same order.  WHMC_REAL: the type theta is cast to (float; the host tool's float64 build of
// the likelihood's arithmetic sets double).
#pragma once
#include "nddm_rng.h"
#include "nddm_wiener_grad.h"

#ifndef WHMC_REAL
#define WHMC_REAL float
#endif

namespace nddm {

typedef WHMC_REAL whmc_real;

constexpr int WHMC_STATE = 12;                  // doubles of state per chain
constexpr int WHMC_MAX_TRIALS = 2048;           // trials of a data set (16 KB of LDS per wave)
constexpr long long WHMC_MAX_ROUNDS = 1ll << 19;    // n_iter * n_leapfrog * ceil(N / 64) of one launch: 1.2 s at the measured 2.3 us a round
                                                    // (profiles/r17_wiener_hmc_rate.json; 2^20 was 2.4 s, too long a hold on a shared GPU)
constexpr double WHMC_DC_MIN = 0.05;
constexpr uint32_t WHMC_TAG = 0x40000000u;
constexpr double WHMC_DELTA = 0.8, WHMC_GAMMA = 0.05, WHMC_T0 = 10.0, WHMC_KAPPA = 0.75;

struct WienerHmcArgs {
    const float *data;          // [D, N, 2]
    double *state;              // [C, WHMC_STATE], in and out
    const double *inv_mass;     // [C, 5] or NULL (ones)
    float *out_draws;           // [C, K, 5] or NULL
    float *out_log_post;        // [C, K] or NULL
    float *out_accept;          // [C] or NULL
    int *out_divergent;         // [C] or NULL
    int *out_flagged;           // [C] or NULL
    long long C, S;             // chains, chains per data set
    unsigned long long chain_offset, iter_offset;
    long long K;                // kept draws per chain
    unsigned k0, k1;            // the seed
    unsigned free_mask;
    int N, n_iter, n_adapt, n_leapfrog, thin;
};

// What a wave learns of its data set while staging it
struct WhmcData {
    double T;                   // min(1.5, smallest rt)
    bool bad;                   // a choice-0 trial, a non-finite value or an rt <= 0
};

// lower limit and width of column j's support (j >= 1)
__device__ __forceinline__ void whmc_support(int j, double T, double &lo, double &wd)
{
    lo = j == 4 ? WHMC_DC_MIN : 0.0;
    wd = j == 1 ? 10.0 : j == 2 ? 1.0 : j == 3 ? T : 10.0 - WHMC_DC_MIN;
}

// sigma(x), log sigma(x), log(1 - sigma(x)) without cancellation at either end
__device__ __forceinline__ void whmc_sigmoid(double x, double &sg, double &lsg, double &l1sg)
{
    const double e = exp(-fabs(x)), l = log1p(e), r = 1.0 / (1.0 + e);
    sg = x >= 0.0 ? r : e * r;
    lsg = x >= 0.0 ? -l : x - l;
    l1sg = x >= 0.0 ? -x - l : -l;
}

// One lane's sums over its trials lane, lane + 64, ... of the data set.  `tile`: the wave's staged trials, all N of them (one tile from 0).
// CENSORED (NDDM_WIENER_CENSORED), here and below: wiener_grad_trial's switch -- a choice-0 trial adds the partials of log S.
template <bool CENSORED = false>
__device__ __forceinline__ WienerGradAcc whmc_lane_sums(const WienerRow &c, const WienerGradRow &g, const float2 *tile, int N, int lane)
{
    WienerGradAcc s = wiener_grad_zero();
    wiener_tile_trials<true, false>(tile, nullptr, 1, N, 0, 0, N, lane,
                                    [&](int, float x0, float x1) { wiener_grad_trial<NDDM_BASIC_DDM_DC, CENSORED>(c, g, x0, x1, s); });
    return s;
}

// The row's six sums over the data set's N trials, every lane's copy alike
#ifndef WHMC_HOST
template <bool CENSORED = false>
__device__ __forceinline__ WienerGradAcc whmc_sums(const WienerRow &c, const WienerGradRow &g, const float2 *tile, int N, int lane)
{
    WienerGradAcc s = whmc_lane_sums<CENSORED>(c, g, tile, N, lane);
    wiener_grad_reduce<NDDM_BASIC_DDM_DC>(s);
    return s;
}

// Lane j stages trials j, j + 64, ... (the ones it reads back) and the wave reduces what it saw.  CENSORED: choice 0 is a trial like the
// others, and T is the smallest rt OF THE RESPONSES (a timeout's rt bounds nothing: tau beyond it leaves log S = 0); no response, T = 1.5.
template <bool CENSORED = false>
__device__ __forceinline__ WhmcData whmc_stage(float2 *tile, const float *src, int N, int lane)
{
    float mn = __builtin_inff();
    bool bad = false;
    for (int i = lane; i < N; i += 64) {
        const float rt = src[2 * i], ch = src[2 * i + 1];
        tile[i] = make_float2(rt, ch);
        bad = bad || !(rt > 0.0f) || !(rt < __builtin_inff()) || !(ch == 1.0f || ch == -1.0f || (CENSORED && ch == 0.0f));
        mn = fminf(mn, CENSORED && ch == 0.0f ? __builtin_inff() : rt);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) mn = fminf(mn, __shfl_xor(mn, m, 64));
    WhmcData d;
    d.bad = __any(bad) != 0;
    d.T = fmin(1.5, (double)mn);
    return d;
}
#else
template <bool CENSORED = false>
inline WienerGradAcc whmc_sums(const WienerRow &c, const WienerGradRow &g, const float2 *tile, int N, int)
{
    WienerGradAcc L[64];
    for (int lane = 0; lane < 64; ++lane) {
        L[lane] = whmc_lane_sums<CENSORED>(c, g, tile, N, lane);
        wiener_grad_fold<NDDM_BASIC_DDM_DC>(L[lane]);
    }
    for (int m = 1; m < 64; m <<= 1)                                    // lane 0's side of the butterfly: the pairwise tree in lane order
        for (int j = 0; j < 64; j += 2 * m) {
            L[j].v += L[j + m].v; L[j].t += L[j + m].t; L[j].a += L[j + m].a; L[j].w += L[j + m].w; L[j].nu += L[j + m].nu;
        }
    return L[0];
}

template <bool CENSORED = false>
inline WhmcData whmc_stage(float2 *tile, const float *src, int N, int)
{
    float mn = __builtin_inff();
    bool bad = false;
    for (int i = 0; i < N; ++i) {
        const float rt = src[2 * i], ch = src[2 * i + 1];
        tile[i] = make_float2(rt, ch);
        bad = bad || !(rt > 0.0f) || !(rt < __builtin_inff()) || !(ch == 1.0f || ch == -1.0f || (CENSORED && ch == 0.0f));
        mn = fminf(mn, CENSORED && ch == 0.0f ? __builtin_inff() : rt);
    }
    WhmcData d;
    d.bad = bad;
    d.T = fmin(1.5, (double)mn);
    return d;
}
#endif

// What a posterior may add to the chain's own: nothing (nddm_wiener_hmc), or nddm_wiener_hmc_joint.h's external measurement of the boundary,
// ext ~ N(boundary, sigma): -(ext - boundary)^2 / (2 sigma^2) on the float64 theta.  `on` is a compile-time switch: the instantiation
// without the term holds none of its arithmetic.
struct WhmcNoExt { static constexpr bool on = false; };
struct WhmcExt {
    static constexpr bool on = true;
    double ext, inv_var;        // the measurement and 1 / sigma^2
};

// log posterior (up to a constant) and its gradient at q, in the unconstrained coordinates; theta: the point in the model's columns
template <class Ext = WhmcNoExt, bool CENSORED = false>
__device__ __forceinline__ double whmc_log_post(const double (&q)[5], unsigned mask, double T, const float2 *tile, int N, int lane,
                                                double (&dq)[5], double (&theta)[5], const Ext &ext = Ext())
{
    double sg[5], jac[5], lj = 0.0;
    theta[0] = q[0]; sg[0] = 0.0; jac[0] = 1.0;
#pragma unroll
    for (int j = 1; j < 5; ++j) {
        if (mask >> j & 1u) {
            double lo, wd, ls, l1s;
            whmc_support(j, T, lo, wd);
            whmc_sigmoid(q[j], sg[j], ls, l1s);
            theta[j] = lo + wd * sg[j];
            jac[j] = wd * sg[j] * (1.0 - sg[j]);
            lj += log(wd) + ls + l1s;
        } else { theta[j] = q[j]; sg[j] = 0.5; jac[j] = 0.0; }
    }
    whmc_real p[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) p[j] = (whmc_real)theta[j];
    const WienerRow c = wiener_row<NDDM_BASIC_DDM_DC>(p);
    const WienerGradRow g = wiener_grad_row<NDDM_BASIC_DDM_DC>(p, c);
    const WienerGradAcc s = whmc_sums<CENSORED>(c, g, tile, N, lane);
    double ll, gl[5];
    wiener_grad_finish<NDDM_BASIC_DDM_DC>(p, c.valid, s, &ll, gl);
    // the priors and their derivatives in theta
    const double v = theta[0], a = theta[1], b = theta[2], ta = theta[3], sc = theta[4];
    double lp = lj;
    if (mask & 1u) { lp += -0.125 * v * v; gl[0] += -0.25 * v; }
    if (mask & 2u) { lp += -2.0 * (a - 1.0) * (a - 1.0); gl[1] += -4.0 * (a - 1.0); }
    if (mask & 4u) { lp += log(b) + log(1.0 - b); gl[2] += 1.0 / b - 1.0 / (1.0 - b); }
    if (mask & 8u) { lp += -8.0 * (ta - 0.5) * (ta - 0.5); gl[3] += -16.0 * (ta - 0.5); }
    if (mask & 16u) { lp += -2.0 * (sc - 1.0) * (sc - 1.0); gl[4] += -4.0 * (sc - 1.0); }
    double le = 0.0;
    if constexpr (Ext::on) {                                            // in theta, before the Jacobian; the value joins the finished sum
        const double d = ext.ext - a;
        le = -0.5 * (d * d) * ext.inv_var;
        gl[1] += d * ext.inv_var;
    }
    dq[0] = (mask & 1u) ? gl[0] : 0.0;
#pragma unroll
    for (int j = 1; j < 5; ++j) dq[j] = (mask >> j & 1u) ? gl[j] * jac[j] + (1.0 - 2.0 * sg[j]) : 0.0;
    if constexpr (Ext::on) return (ll + lp) + le;
    return ll + lp;
}

// Five standard normals and two uniforms in (0, 1) of (seed, global chain, global iteration)
__device__ __forceinline__ void whmc_randoms(unsigned k0, unsigned k1, unsigned chain, unsigned iter, float (&z)[5], float &u1, float &u2)
{
    float z4[4];
    normals4<false>(chain, iter, WHMC_TAG, WHMC_TAG, k0, k1, z4);
    z[0] = z4[0]; z[1] = z4[1]; z[2] = z4[2]; z[3] = z4[3];
    const u32x4 x = philox4x32_10(chain, iter, WHMC_TAG | 1u, WHMC_TAG, k0, k1);
    float r, cs, sn;
    polar_pair<false>(x.x, x.y, r, cs, sn);
    z[4] = r * cs;
    u1 = uniform01(x.z);
    u2 = uniform01(x.w);
}

// What a chain hands back of a launch beside its state and its kept draws
struct WhmcTally {
    double accept_sum;          // sum of the acceptance probabilities of the non-adapting iterations
    int n_sampling, n_divergent;
};

// One chain through iterations [iter_offset, iter_offset + n_iter): st is its state (updated), im its inverse mass; kept draws go to
// draws / log_post (either may be NULL) through `keep` (lane 0 on the device).  The data set is staged in `tile`.  `ext`: see WhmcNoExt.
template <class Ext = WhmcNoExt, bool CENSORED = false>
__device__ __forceinline__ WhmcTally whmc_chain(double *st, const double (&im)[5], const float2 *tile, int N, double T, unsigned mask,
                                                unsigned k0, unsigned k1, unsigned chain, unsigned long long iter_offset, int n_iter,
                                                int n_adapt, int n_leapfrog, int thin, float *draws, float *log_post, int lane, bool keep,
                                                const Ext &ext = Ext())
{
    double q[5], g[5], th[5], sim[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) { q[j] = st[j]; sim[j] = sqrt(im[j]); }
    double leps = st[5], lbar = st[6], hbar = st[7];
    const double mu = st[8];
    double adapted = st[9], elast = st[10], emax = st[11];
    double lp = whmc_log_post<Ext, CENSORED>(q, mask, T, tile, N, lane, g, th, ext);
    WhmcTally tally = {0.0, 0, 0};
    long long kept = 0;
    for (int it = 0; it < n_iter; ++it) {
        const unsigned long long gi = iter_offset + (unsigned long long)it;
        float z[5], u1, u2;
        whmc_randoms(k0, k1, chain, (unsigned)gi, z, u1, u2);
        const double eps = exp(leps) * (0.8 + 0.2 * (double)u1);
        double p[5], qn[5], gn[5], thn[5], kin = 0.0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            p[j] = (mask >> j & 1u) ? (double)z[j] / sim[j] : 0.0;
            kin += 0.5 * im[j] * p[j] * p[j];
            qn[j] = q[j]; gn[j] = g[j]; thn[j] = th[j];
        }
        const double H0 = -lp + kin;
        double lpn = lp;
        for (int l = 0; l < n_leapfrog; ++l) {
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                p[j] += 0.5 * eps * gn[j];
                qn[j] += eps * im[j] * p[j];
            }
            lpn = whmc_log_post<Ext, CENSORED>(qn, mask, T, tile, N, lane, gn, thn, ext);
#pragma unroll
            for (int j = 0; j < 5; ++j) p[j] += 0.5 * eps * gn[j];
        }
        kin = 0.0;
#pragma unroll
        for (int j = 0; j < 5; ++j) kin += 0.5 * im[j] * p[j] * p[j];
        const double H1 = -lpn + kin, d = H0 - H1;
        const bool divergent = !(fabs(H1) < (double)__builtin_inff()) || H1 - H0 > 1000.0;
        const bool usable = !divergent && d == d;
        const double alpha = usable ? fmin(1.0, exp(d)) : 0.0;
        const bool accept = usable && log((double)u2) < d;
        tally.n_divergent += divergent ? 1 : 0;
        elast = H1 - H0;
        emax = fabs(elast) < (double)__builtin_inff() ? fmax(emax, fabs(elast)) : emax;
        if (accept) {
            lp = lpn;
#pragma unroll
            for (int j = 0; j < 5; ++j) { q[j] = qn[j]; g[j] = gn[j]; th[j] = thn[j]; }
        }
        if (adapted < (double)n_adapt) {
            adapted += 1.0;
            const double w = 1.0 / (adapted + WHMC_T0), x = exp(-WHMC_KAPPA * log(adapted));       // m^-kappa
            hbar = (1.0 - w) * hbar + w * (WHMC_DELTA - alpha);
            leps = mu - sqrt(adapted) / WHMC_GAMMA * hbar;
            lbar = x * leps + (1.0 - x) * lbar;
            if (!(adapted < (double)n_adapt)) leps = lbar;
        } else {
            tally.accept_sum += alpha;
            tally.n_sampling += 1;
        }
        if ((gi + 1ull) % (unsigned long long)thin == 0ull) {
            if (keep) {
                if (draws) {
#pragma unroll
                    for (int j = 0; j < 5; ++j) draws[kept * 5 + j] = (float)th[j];
                }
                if (log_post) log_post[kept] = (float)lp;
            }
            ++kept;
        }
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) st[j] = q[j];
    st[5] = leps; st[6] = lbar; st[7] = hbar; st[9] = adapted; st[10] = elast; st[11] = emax;
    return tally;
}

// the incoming state and inverse mass a chain can run from: finite, the masses positive
__device__ __forceinline__ bool whmc_state_ok(const double *st, const double (&im)[5])
{
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 10; ++j) ok = ok && fabs(st[j]) < (double)__builtin_inff();
#pragma unroll
    for (int j = 0; j < 5; ++j) ok = ok && im[j] > 0.0 && im[j] < (double)__builtin_inff();
    return ok;
}

#ifndef WHMC_HOST
// The kernel's body (the workgroup's 4 x WHMC_MAX_TRIALS pairs of LDS are declared in it: each kernel gets its own)
template <bool CENSORED>
__device__ __forceinline__ void wiener_hmc_body(const WienerHmcArgs &A)
{
    __shared__ float2 tiles[4 * WHMC_MAX_TRIALS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long c = (long long)blockIdx.x * 4 + wave;
    if (c >= A.C) return;                                               // wave-uniform; no barrier follows
    float2 *tile = tiles + wave * WHMC_MAX_TRIALS;
    const WhmcData dat = whmc_stage<CENSORED>(tile, A.data + (c / A.S) * (long long)A.N * 2, A.N, lane);
    double st[WHMC_STATE], im[5];
#pragma unroll
    for (int j = 0; j < WHMC_STATE; ++j) st[j] = A.state[c * WHMC_STATE + j];
#pragma unroll
    for (int j = 0; j < 5; ++j) im[j] = A.inv_mass ? A.inv_mass[c * 5 + j] : 1.0;
    float *draws = A.out_draws ? A.out_draws + c * A.K * 5 : nullptr;
    float *log_post = A.out_log_post ? A.out_log_post + c * A.K : nullptr;
    if (dat.bad || !whmc_state_ok(st, im)) {
        const float nan = __builtin_nanf("");
        if (draws) for (long long i = lane; i < A.K * 5; i += 64) draws[i] = nan;
        if (log_post) for (long long i = lane; i < A.K; i += 64) log_post[i] = nan;
        if (lane == 0) {
            if (A.out_accept) A.out_accept[c] = nan;
            if (A.out_divergent) A.out_divergent[c] = 0;
            if (A.out_flagged) A.out_flagged[c] = 1;
        }
        return;
    }
    const WhmcTally t = whmc_chain<WhmcNoExt, CENSORED>(st, im, tile, A.N, dat.T, A.free_mask, A.k0, A.k1,
                                                        (unsigned)(A.chain_offset + (unsigned long long)c), A.iter_offset, A.n_iter, A.n_adapt,
                                                        A.n_leapfrog, A.thin, draws, log_post, lane, lane == 0);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < WHMC_STATE; ++j) A.state[c * WHMC_STATE + j] = st[j];
        if (A.out_accept) A.out_accept[c] = t.n_sampling ? (float)(t.accept_sum / (double)t.n_sampling) : __builtin_nanf("");
        if (A.out_divergent) A.out_divergent[c] = t.n_divergent;
        if (A.out_flagged) A.out_flagged[c] = 0;
    }
}

__global__ __launch_bounds__(256) void wiener_hmc_kernel(WienerHmcArgs A)
{
    wiener_hmc_body<false>(A);
}

// NDDM_WIENER_CENSORED: the same chain with timeouts scored (a kernel of its own: wiener_hmc_kernel holds none of the survival code)
__global__ __launch_bounds__(256) void wiener_hmc_censored_kernel(WienerHmcArgs A)
{
    wiener_hmc_body<true>(A);
}
#endif

}  // namespace nddm
