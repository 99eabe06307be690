// nddm_wiener_hmc_joint.h -- the alpha_not_scaled JAGS fit (alpha_not_scaled.py:138-259, jagscode/alpha_not_scaled_test2.jags) on the
// device (gfx950): every participant p has (delta, alpha, beta, ndt, varsigma) under nddm_wiener_hmc.h's posterior, an external measurement
// ext_p ~ N(alpha_p, sigma) of the boundary, and ONE sigma ~ N(3, 1) T(0, 10) shared by all participants.  Metropolis within Gibbs: given
// sigma the participants are independent and their log posterior is nddm_wiener_hmc.h's plus -(ext_p - alpha_p)^2 / (2 sigma^2); given the
// participants sigma has a one-dimensional conditional.  Included by nddm_kernels.hip after nddm_wiener_hmc.h, whose whmc_chain is CALLED
// (one iteration at a time), not copied.  DESIGN.md section 18.
//
// Layout: P participants, S joint chains; participant chain c = p S + k (nddm_wiener_hmc.h's: chain c reads data set c / S), state double
// [P S, WHMC_STATE], sigma double [S] in and out.  Joint iteration g of joint chain k:
//   1. participant update, one wave per (p, k): whmc_chain<WhmcExt> with n_iter = 1 -- the Philox stream is that chain's own (chain index
//      chain_offset + c, iteration g, WHMC_TAG).  alpha_p in the ext term is the float64 theta, not the float32 cast the likelihood sees; the
//      term is in the log posterior whether or not the boundary is free.
//   2. sigma update, one wave per k: SS = sum_p (ext_p - alpha_p)^2 in float64 (lanes stride over p, a butterfly reduces: the bits do not
//      depend on the grid), alpha_p = 10 sigmoid(q1) of chain (p, k)'s state, or q1 itself where the boundary is fixed.  An independence
//      Metropolis step: chi2 = the sum of squares of P - 1 standard normals (the EXACT Box-Muller of nddm_rng.h; lane j takes Philox blocks
//      j, j + 64, ..., the surplus normals of the last block unused), sigma' = sqrt(SS / chi2) -- a draw from the likelihood part of the
//      conditional, sigma^-P exp(-SS / 2 sigma^2) -- accepted when sigma' is finite and in (0, 10) and
//      log u < -(sigma' - 3)^2 / 2 + (sigma - 3)^2 / 2.  Stream: key = seed, counter (chain_offset + k, g, WHMCJ_TAG | block, WHMCJ_TAG); no
//      stream of DESIGN.md section 4 has that tag (1, 2, 4 and 8 in the top nibble are taken; this is 5).  u: the block after the last normal one.
// The kept draw of iteration g is taken after both parts when (g + 1) % thin == 0.
//
// THE COUPLING IS BY LAUNCH ORDER, NOT BY WAITING: per iteration the entry point enqueues wiener_hmc_joint_kernel and then
// wiener_hmc_joint_sigma_kernel on the caller's stream.  No host synchronisation between iterations, no cooperative launch or grid sync, no
// spinning on memory between workgroups, no atomics; every store is a plain vector store.  (A persistent kernel cannot do this safely on a
// shared card: the reference's 600 waves would have to meet every iteration, and a wave that is not resident never arrives.)  The
// participant kernel stages its data set into LDS again each launch and evaluates the log posterior at the incoming q: one gradient more per
// iteration than nddm_wiener_hmc (n_leapfrog + 1 against n_leapfrog).
//
// Before the first iteration ONE pre-pass workgroup validates by reading values and clears the call's accumulators in `workspace`, double
// [P S + S, 4]: row c = (sum of acceptance probabilities, sampling iterations, divergent iterations, -) of participant chain c, row P S + k =
// (accepted sigma proposals, -, flagged, -) of joint chain k.  (T = min(1.5, smallest rt) is found by the participant wave while it stages,
// as in nddm_wiener_hmc.h: the pre-pass has no reader for it.)  A data set with a choice-0 trial, a non-finite value or an rt <= 0 flags EVERY
// chain of the call (every joint chain contains it); joint chain k alone is flagged when the incoming state or inverse mass of any (p, k) is
// not finite, or sigma_k is not finite and > 0, or not < 10 when sampled.  A flagged joint chain runs no iteration: sigma and states
// unchanged, draws NaN, flagged = 1 for its P chains; the other joint chains' bits are unaffected.
//
// A joint chain's output is a pure function of (seed, chain_offset, k, S, all P data sets and ext, its P incoming states and inv_mass, its
// sigma, free_mask, flags, n_leapfrog, thin, n_adapt, the iteration range): not of the grid, the other joint chains, or how the range is cut.
//
// WHMC_HOST: tools/wiener_hmc_joint_host.py compiles whmcj_participant and whmcj_sigma_step for the host, lanes as loops, the butterfly in
// the kernel's order.
#pragma once
#include "nddm_wiener_hmc.h"

namespace nddm {

constexpr uint32_t WHMCJ_TAG = 0x50000000u;
constexpr int WHMCJ_MAX_ITER = 4096;            // joint iterations of one call: 2 x 4096 + 1 kernel nodes
constexpr int WHMCJ_WS = 4;                     // doubles per workspace row

struct WienerHmcJointArgs {
    const float *data;          // [P, N, 2]
    const double *ext;          // [P]
    double *state;              // [P S, WHMC_STATE], in and out
    const double *inv_mass;     // [P S, 5] or NULL (ones)
    double *sigma;              // [S], in and out
    double *ws;                 // [P S + S, WHMCJ_WS]
    float *out_draws;           // [P S, K, 5] or NULL
    float *out_log_post;        // [P S, K] or NULL
    float *out_accept;          // [P S] or NULL
    int *out_divergent;         // [P S] or NULL
    int *out_flagged;           // [P S] or NULL
    float *out_sigma;           // [S, K] or NULL
    float *out_sigma_accept;    // [S] or NULL
    long long P, S;
    unsigned long long chain_offset, iter_offset;
    long long K;
    unsigned k0, k1;
    unsigned free_mask;
    int N, n_iter, n_adapt, n_leapfrog, thin;
    int sigma_fixed;
    int it;                     // the launch's iteration of the call, 0 .. n_iter - 1
    int censored;               // NDDM_WIENER_CENSORED: what the pre-pass takes for a trial (the participant kernel is the censored one)
};

// f(lane) summed over the 64 lanes in the butterfly's order (every lane's copy alike on the device; lane 0's side of the tree on the host)
#ifndef WHMC_HOST
template <class F>
__device__ __forceinline__ double whmcj_wave_sum(F f, int lane)
{
    double x = f(lane);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m, 64);
    return x;
}
#else
template <class F>
inline double whmcj_wave_sum(F f, int)
{
    double L[64];
    for (int lane = 0; lane < 64; ++lane) L[lane] = f(lane);
    for (int m = 1; m < 64; m <<= 1)
        for (int j = 0; j < 64; j += 2 * m) L[j] += L[j + m];
    return L[0];
}
#endif

// the boundary a chain's state holds: whmc_log_post's theta[1]
__device__ __forceinline__ double whmcj_alpha(const double *st, unsigned mask)
{
    if (!(mask & 2u)) return st[1];
    double lo, wd, sg, ls, l1s;
    whmc_support(1, 0.0, lo, wd);
    whmc_sigmoid(st[1], sg, ls, l1s);
    return lo + wd * sg;
}

// SS of joint chain k from the P states of its participants
__device__ __forceinline__ double whmcj_ss(const double *state, const double *ext, long long P, long long S, long long k, unsigned mask, int lane)
{
    return whmcj_wave_sum([=](int ln) {
        double s = 0.0;
        for (long long p = ln; p < P; p += 64) {
            const double d = ext[p] - whmcj_alpha(state + (p * S + k) * WHMC_STATE, mask);
            s += d * d;
        }
        return s;
    }, lane);
}

// the sum of squares of n standard normals of (seed, chain, iteration): blocks 0 .. ceil(n / 4) - 1 of the sigma stream
__device__ __forceinline__ double whmcj_chi2(unsigned k0, unsigned k1, unsigned chain, unsigned iter, long long n, int lane)
{
    const long long nb = (n + 3) / 4;
    return whmcj_wave_sum([=](int ln) {
        double s = 0.0;
        for (long long b = ln; b < nb; b += 64) {
            float z[4];
            normals4<false>(chain, iter, WHMCJ_TAG | (uint32_t)b, WHMCJ_TAG, k0, k1, z);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * b + j < n) s += (double)z[j] * (double)z[j];
        }
        return s;
    }, lane);
}

// PART 2: the sigma update of joint chain `chain` at iteration `iter` given SS -> accepted (sigma updated)
__device__ __forceinline__ bool whmcj_sigma_step(double &sigma, double SS, long long P, unsigned k0, unsigned k1, unsigned chain, unsigned iter,
                                                 int lane)
{
    const double chi2 = whmcj_chi2(k0, k1, chain, iter, P - 1, lane);
    const double sp = sqrt(SS / chi2);
    const u32x4 x = philox4x32_10(chain, iter, WHMCJ_TAG | (uint32_t)((P - 1 + 3) / 4), WHMCJ_TAG, k0, k1);
    const double lu = log((double)uniform01(x.x));
    const bool accept = sp > 0.0 && sp < 10.0 && lu < -0.5 * (sp - 3.0) * (sp - 3.0) + 0.5 * (sigma - 3.0) * (sigma - 3.0);
    if (accept) sigma = sp;
    return accept;
}

// PART 1: iteration gi of participant chain `chain` given sigma: one iteration of nddm_wiener_hmc.h's chain with the ext term.  draws /
// log_post: where THIS iteration's kept draw goes (read only when (gi + 1) % thin == 0).  CENSORED: nddm_wiener_hmc.h's switch, passed through.
template <bool CENSORED = false>
__device__ __forceinline__ WhmcTally whmcj_participant(double *st, const double (&im)[5], const float2 *tile, int N, double T, unsigned mask,
                                                       unsigned k0, unsigned k1, unsigned chain, unsigned long long gi, int n_adapt,
                                                       int n_leapfrog, int thin, float *draws, float *log_post, int lane, bool keep,
                                                       double ext, double sigma)
{
    const WhmcExt e = {ext, 1.0 / (sigma * sigma)};
    return whmc_chain<WhmcExt, CENSORED>(st, im, tile, N, T, mask, k0, k1, chain, gi, 1, n_adapt, n_leapfrog, thin, draws, log_post, lane, keep, e);
}

// the sigma a joint chain can run from
__device__ __forceinline__ bool whmcj_sigma_ok(double sigma, bool fixed)
{
    return sigma > 0.0 && sigma < (double)__builtin_inff() && (fixed || sigma < 10.0);
}

// the slot of iteration gi's kept draw among the call's K (only when (gi + 1) % thin == 0)
__device__ __forceinline__ long long whmcj_slot(unsigned long long gi, unsigned long long iter_offset, int thin)
{
    return (long long)((gi + 1ull) / (unsigned long long)thin - iter_offset / (unsigned long long)thin) - 1;
}

#ifndef WHMC_HOST
// One workgroup: validate, clear the accumulators, write what a flagged (or sigma-fixed) joint chain reports.
__global__ __launch_bounds__(256) void wiener_hmc_joint_prepass_kernel(WienerHmcJointArgs A)
{
    __shared__ int s_bad[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool bad = false;
    for (long long p = wave; p < A.P; p += 4) {
        const float *src = A.data + p * (long long)A.N * 2;
        for (int i = lane; i < A.N; i += 64) {
            const float rt = src[2 * i], ch = src[2 * i + 1];
            bad = bad || !(rt > 0.0f) || !(rt < __builtin_inff()) || !(ch == 1.0f || ch == -1.0f || (A.censored && ch == 0.0f));
        }
    }
    bad = __any(bad) != 0;
    if (lane == 0) s_bad[wave] = bad;
    __syncthreads();
    const bool any_bad = (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) != 0;
    const float nan = __builtin_nanf("");
    const long long C = A.P * A.S;
    for (long long k = wave; k < A.S; k += 4) {                         // wave-uniform
        bool f = false;
        for (long long p = lane; p < A.P; p += 64) {
            const long long c = p * A.S + k;
            double st[WHMC_STATE], im[5];
#pragma unroll
            for (int j = 0; j < WHMC_STATE; ++j) st[j] = A.state[c * WHMC_STATE + j];
#pragma unroll
            for (int j = 0; j < 5; ++j) im[j] = A.inv_mass ? A.inv_mass[c * 5 + j] : 1.0;
            f = f || !whmc_state_ok(st, im);
        }
        const double sg = A.sigma[k];
        const bool flagged = __any(f) != 0 || any_bad || !whmcj_sigma_ok(sg, A.sigma_fixed != 0);
        for (long long p = lane; p < A.P; p += 64) {
            const long long c = p * A.S + k;
#pragma unroll
            for (int j = 0; j < WHMCJ_WS; ++j) A.ws[c * WHMCJ_WS + j] = 0.0;
            if (A.out_flagged) A.out_flagged[c] = flagged ? 1 : 0;
            if (flagged && A.out_accept) A.out_accept[c] = nan;
            if (flagged && A.out_divergent) A.out_divergent[c] = 0;
        }
        if (flagged) {
            for (long long p = 0; p < A.P; ++p) {
                const long long c = p * A.S + k;
                if (A.out_draws) for (long long i = lane; i < A.K * 5; i += 64) A.out_draws[c * A.K * 5 + i] = nan;
                if (A.out_log_post) for (long long i = lane; i < A.K; i += 64) A.out_log_post[c * A.K + i] = nan;
            }
        }
        if (A.out_sigma && (flagged || A.sigma_fixed))
            for (long long i = lane; i < A.K; i += 64) A.out_sigma[k * A.K + i] = flagged ? nan : (float)sg;
        if (lane == 0) {
            double *w = A.ws + (C + k) * WHMCJ_WS;
            w[0] = 0.0; w[1] = 0.0; w[2] = flagged ? 1.0 : 0.0; w[3] = 0.0;
            if (A.out_sigma_accept && (flagged || A.sigma_fixed)) A.out_sigma_accept[k] = nan;
        }
    }
}

// PART 1 of iteration A.it: 256 threads = 4 waves = 4 participant chains per workgroup, as wiener_hmc_kernel.  The body (the
// workgroup's LDS is declared in it: each kernel gets its own)
template <bool CENSORED>
__device__ __forceinline__ void wiener_hmc_joint_body(const WienerHmcJointArgs &A)
{
    __shared__ float2 tiles[4 * WHMC_MAX_TRIALS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long C = A.P * A.S, c = (long long)blockIdx.x * 4 + wave;
    if (c >= C) return;                                                 // wave-uniform; no barrier follows
    const long long p = c / A.S, k = c % A.S;
    if (A.ws[(C + k) * WHMCJ_WS + 2] != 0.0) return;                    // a flagged joint chain runs no iteration
    float2 *tile = tiles + wave * WHMC_MAX_TRIALS;
    const WhmcData dat = whmc_stage<CENSORED>(tile, A.data + p * (long long)A.N * 2, A.N, lane);
    double st[WHMC_STATE], im[5];
#pragma unroll
    for (int j = 0; j < WHMC_STATE; ++j) st[j] = A.state[c * WHMC_STATE + j];
#pragma unroll
    for (int j = 0; j < 5; ++j) im[j] = A.inv_mass ? A.inv_mass[c * 5 + j] : 1.0;
    const unsigned long long gi = A.iter_offset + (unsigned long long)A.it;
    const bool kept = (gi + 1ull) % (unsigned long long)A.thin == 0ull;
    const long long slot = kept ? whmcj_slot(gi, A.iter_offset, A.thin) : 0;
    float *draws = kept && A.out_draws ? A.out_draws + (c * A.K + slot) * 5 : nullptr;
    float *log_post = kept && A.out_log_post ? A.out_log_post + c * A.K + slot : nullptr;
    const WhmcTally t = whmcj_participant<CENSORED>(st, im, tile, A.N, dat.T, A.free_mask, A.k0, A.k1, (unsigned)(A.chain_offset + (unsigned long long)c), gi,
                                          A.n_adapt, A.n_leapfrog, A.thin, draws, log_post, lane, lane == 0, A.ext[p], A.sigma[k]);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < WHMC_STATE; ++j) A.state[c * WHMC_STATE + j] = st[j];
        double *w = A.ws + c * WHMCJ_WS;
        const double acc = w[0] + t.accept_sum, ns = w[1] + (double)t.n_sampling, nd = w[2] + (double)t.n_divergent;
        w[0] = acc; w[1] = ns; w[2] = nd;
        if (A.it == A.n_iter - 1) {
            if (A.out_accept) A.out_accept[c] = ns > 0.0 ? (float)(acc / ns) : __builtin_nanf("");
            if (A.out_divergent) A.out_divergent[c] = (int)nd;
        }
    }
}

__global__ __launch_bounds__(256) void wiener_hmc_joint_kernel(WienerHmcJointArgs A)
{
    wiener_hmc_joint_body<false>(A);
}

// NDDM_WIENER_CENSORED's participant kernel (a kernel of its own: wiener_hmc_joint_kernel holds none of the survival code)
__global__ __launch_bounds__(256) void wiener_hmc_censored_joint_kernel(WienerHmcJointArgs A)
{
    wiener_hmc_joint_body<true>(A);
}

// PART 2 of iteration A.it: one wave per joint chain
__global__ __launch_bounds__(256) void wiener_hmc_joint_sigma_kernel(WienerHmcJointArgs A)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long C = A.P * A.S, k = (long long)blockIdx.x * 4 + wave;
    if (k >= A.S) return;
    double *w = A.ws + (C + k) * WHMCJ_WS;
    if (w[2] != 0.0) return;
    const unsigned long long gi = A.iter_offset + (unsigned long long)A.it;
    double sg = A.sigma[k];
    const double SS = whmcj_ss(A.state, A.ext, A.P, A.S, k, A.free_mask, lane);
    const bool accept = whmcj_sigma_step(sg, SS, A.P, A.k0, A.k1, (unsigned)(A.chain_offset + (unsigned long long)k), (unsigned)gi, lane);
    if (lane == 0) {
        const double na = w[0] + (accept ? 1.0 : 0.0);
        w[0] = na;
        A.sigma[k] = sg;
        if (A.out_sigma && (gi + 1ull) % (unsigned long long)A.thin == 0ull) A.out_sigma[k * A.K + whmcj_slot(gi, A.iter_offset, A.thin)] = (float)sg;
        if (A.out_sigma_accept && A.it == A.n_iter - 1) A.out_sigma_accept[k] = (float)(na / (double)A.n_iter);
    }
}
#endif

}  // namespace nddm
