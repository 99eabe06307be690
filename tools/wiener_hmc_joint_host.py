#!/usr/bin/env python3
"""The joint sampler of csrc/nddm_wiener_hmc_joint.h run on the HOST, without a GPU: the header's own whmcj_participant (one iteration of
nddm_wiener_hmc.h's chain with the ext term) and whmcj_sigma_step (with whmcj_ss), compiled by the host compiler as a stand-alone program
the way tools/wiener_hmc_host.py compiles the independent chain -- the 64 lanes as loops, the butterflies in the kernel's order -- and
driven in the entry point's order: the pre-pass's flags, then per iteration every participant of a joint chain and its sigma step.  Two
builds: float32 (the kernel's arithmetic) and `f64=True` (the likelihood's headers with every float a double).

run(exe, td, data [P, N, 2], extdata [P], state [P S, 12], sigma [S], ...) -> dict with the C entry point's outputs, the updated state
and sigma.

Usage: python tools/wiener_hmc_joint_host.py [--sanitize] [--json OUT]      prints one JSON line: the energy error of short trajectories
with the ext term on (sigma = 0.2) at eps = 1e-3 (the bar of the energy tests = 4 x the largest, per shape), and float32 against float64
over 3 iterations of 4 leapfrog steps for every case of the device-against-host test (its tolerance = 4 x that case's difference).
--sanitize runs one small case through a build under AddressSanitizer and UndefinedBehaviorSanitizer first (a stand-alone program).
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wiener_hmc_host as H  # noqa: E402  (the shims, the cases, the comparison)
import host_build as B  # noqa: E402  (the stand-in header, the compiler call, the command line)

STATE = H.STATE
SIGMA_FIXED = 1

MAIN = r"""// usage: wiener_hmc_joint_host in.bin out.bin ; in: 13 int64 (P, N, S, n_iter, n_adapt, n_leapfrog, thin, free_mask, seed, chain_offset,
// iter_offset, has_inv_mass, flags), data f32 [P, N, 2], ext f64 [P], state f64 [C, 12], sigma f64 [S], inv_mass f64 [C, 5] if has_inv_mass;
// out: draws f32 [C, K, 5], log_post f32 [C, K], accept f32 [C], divergent i32 [C], flagged i32 [C], sigma draws f32 [S, K], sigma accept
// f32 [S], state f64 [C, 12], sigma f64 [S]
#include <cstdio>
#include <cstdlib>
#include <vector>
%s
#include "nddm_wiener_hmc_joint.h"
using namespace nddm;
int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb"); long long h[13]; if (!f || fread(h, 8, 13, f) != 13) return 2;
    const long long P = h[0], N = h[1], S = h[2], n_iter = h[3], n_adapt = h[4], L = h[5], thin = h[6], C = P * S;
    const unsigned mask = (unsigned)h[7]; const unsigned long long seed = (unsigned long long)h[8], coff = h[9], ioff = h[10];
    const bool fixed = (h[12] & 1) != 0;
    if (N > WHMC_MAX_TRIALS || N <= 0 || P <= 0 || S <= 0 || n_iter > WHMCJ_MAX_ITER || n_iter * L * ((N + 63) / 64) > WHMC_MAX_ROUNDS ||
        (!fixed && P < 2)) return 5;
    const long long K = (long long)((ioff + n_iter) / thin - ioff / thin);
    const float nanf_ = __builtin_nanf("");
    std::vector<float> data((size_t)P * N * 2), draws((size_t)C * K * 5), lpost((size_t)C * K), acc(C), sdraws((size_t)S * K), sacc(S);
    std::vector<double> ext(P), state((size_t)C * WHMC_STATE), sigma(S), im((size_t)C * 5, 1.0);
    std::vector<int> dv(C), fl(C);
    if (fread(data.data(), 4, data.size(), f) != data.size()) return 3;
    if (fread(ext.data(), 8, ext.size(), f) != ext.size()) return 3;
    if (fread(state.data(), 8, state.size(), f) != state.size()) return 3;
    if (fread(sigma.data(), 8, sigma.size(), f) != sigma.size()) return 3;
    if (h[11] && fread(im.data(), 8, im.size(), f) != im.size()) return 3;
    fclose(f);
    // the pre-pass: the staged data sets, T, and whether any of them is bad
    std::vector<std::vector<float2>> tiles(P, std::vector<float2>(N));
    std::vector<double> T(P);
    bool any_bad = false;
    for (long long p = 0; p < P; ++p) {
        const WhmcData d = whmc_stage<HOST_CENSORED>(tiles[p].data(), data.data() + p * N * 2, (int)N, 0);
        T[p] = d.T; any_bad = any_bad || d.bad;
    }
    for (long long k = 0; k < S; ++k) {
        bool flagged = any_bad || !whmcj_sigma_ok(sigma[k], fixed);
        for (long long p = 0; p < P; ++p) {
            double m[5];
            for (int j = 0; j < 5; ++j) m[j] = im[(p * S + k) * 5 + j];
            flagged = flagged || !whmc_state_ok(&state[(p * S + k) * WHMC_STATE], m);
        }
        for (long long p = 0; p < P; ++p) fl[p * S + k] = flagged;
        if (flagged) {
            for (long long p = 0; p < P; ++p) {
                const long long c = p * S + k;
                for (long long i = 0; i < K * 5; ++i) draws[c * K * 5 + i] = nanf_;
                for (long long i = 0; i < K; ++i) lpost[c * K + i] = nanf_;
                acc[c] = nanf_; dv[c] = 0;
            }
            for (long long i = 0; i < K; ++i) sdraws[k * K + i] = nanf_;
            sacc[k] = nanf_;
            continue;
        }
        std::vector<double> w((size_t)P * 3, 0.0);
        double na = 0.0;
        for (long long it = 0; it < n_iter; ++it) {
            const unsigned long long gi = ioff + it;
            const bool kept = (gi + 1) %% (unsigned long long)thin == 0;
            const long long slot = kept ? whmcj_slot(gi, ioff, (int)thin) : 0;
            for (long long p = 0; p < P; ++p) {
                const long long c = p * S + k;
                double m[5];
                for (int j = 0; j < 5; ++j) m[j] = im[c * 5 + j];
                const WhmcTally t = whmcj_participant<HOST_CENSORED>(&state[c * WHMC_STATE], m, tiles[p].data(), (int)N, T[p], mask, (unsigned)seed,
                                                      (unsigned)(seed >> 32), (unsigned)(coff + c), gi, (int)n_adapt, (int)L, (int)thin,
                                                      kept ? &draws[(c * K + slot) * 5] : nullptr, kept ? &lpost[c * K + slot] : nullptr, 0, true,
                                                      ext[p], sigma[k]);
                w[p * 3] += t.accept_sum; w[p * 3 + 1] += (double)t.n_sampling; w[p * 3 + 2] += (double)t.n_divergent;
            }
            if (!fixed) {
                const double SS = whmcj_ss(state.data(), ext.data(), P, S, k, mask, 0);
                na += whmcj_sigma_step(sigma[k], SS, P, (unsigned)seed, (unsigned)(seed >> 32), (unsigned)(coff + k), (unsigned)gi, 0) ? 1.0 : 0.0;
            }
            if (kept) sdraws[k * K + slot] = (float)sigma[k];
        }
        for (long long p = 0; p < P; ++p) {
            acc[p * S + k] = w[p * 3 + 1] > 0.0 ? (float)(w[p * 3] / w[p * 3 + 1]) : nanf_;
            dv[p * S + k] = (int)w[p * 3 + 2];
        }
        sacc[k] = fixed ? nanf_ : (float)(na / (double)n_iter);
    }
    f = fopen(argv[2], "wb"); if (!f) return 4;
    fwrite(draws.data(), 4, draws.size(), f); fwrite(lpost.data(), 4, lpost.size(), f); fwrite(acc.data(), 4, acc.size(), f);
    fwrite(dv.data(), 4, dv.size(), f); fwrite(fl.data(), 4, fl.size(), f); fwrite(sdraws.data(), 4, sdraws.size(), f);
    fwrite(sacc.data(), 4, sacc.size(), f); fwrite(state.data(), 8, state.size(), f); fwrite(sigma.data(), 8, sigma.size(), f);
    fclose(f);
    return 0;
}
"""


def build(td, sanitize=False, f64=False, censored=False):
    """Compile the stand-alone program into a directory of its own under td -> its path.  censored: NDDM_WIENER_CENSORED's chains."""
    sub = os.path.join(td, ("j64" if f64 else "j32") + ("s" if sanitize else "") + ("_censored" if censored else ""))
    os.makedirs(sub)
    switch = "#define HOST_CENSORED %s\n" % ("true" if censored else "false")
    return B.build(sub, MAIN % (switch + H.RNG_SHIM + (H.F64_ON if f64 else "")), "wiener_hmc_joint_host", sanitize)


kept = H.kept


def run(exe, td, data, extdata, state, sigma, inv_mass=None, n_iter=1, n_adapt=0, n_leapfrog=16, thin=1, free_mask=31, seed=0, chain_offset=0,
        iter_offset=0, sigma_fixed=False):
    """The C entry point's call on the host -> {'draws' [C, K, 5], 'log_post' [C, K], 'accept' [C], 'divergent' [C], 'flagged' [C],
    'sigma_draws' [S, K], 'sigma_accept' [S], 'state' [C, 12], 'sigma' [S]} (numpy; state and sigma are new arrays)."""
    data = np.ascontiguousarray(data, np.float32)
    state = np.ascontiguousarray(state, np.float64)
    sigma = np.ascontiguousarray(sigma, np.float64).reshape(-1)
    extdata = np.ascontiguousarray(extdata, np.float64).reshape(-1)
    P, N, _ = data.shape
    S = sigma.shape[0]
    C = P * S
    assert state.shape == (C, STATE) and extdata.shape == (P,)
    K = kept(iter_offset, n_iter, thin)
    return B.exchange(exe, [P, N, S, n_iter, n_adapt, n_leapfrog, thin, free_mask, seed, chain_offset, iter_offset, inv_mass is not None,
                            SIGMA_FIXED if sigma_fixed else 0],
                      [data, extdata, state, sigma] + ([] if inv_mass is None else [np.ascontiguousarray(inv_mass, np.float64).reshape(C, 5)]),
                      (("draws", np.float32, (C, K, 5)), ("log_post", np.float32, (C, K)), ("accept", np.float32, (C,)),
                       ("divergent", np.int32, (C,)), ("flagged", np.int32, (C,)), ("sigma_draws", np.float32, (S, K)),
                       ("sigma_accept", np.float32, (S,)), ("state", np.float64, (C, STATE)), ("sigma", np.float64, (S,))))


PROFILE = os.path.join(ROOT, "profiles", "r18_wiener_hmc_joint_host.json")
ENERGY_SHAPES = H.ENERGY_SHAPES
ENERGY = dict(H.ENERGY, sigma_fixed=True)           # at eps0 = 1e-3, no adaptation, sigma held at ENERGY_SIGMA
ENERGY_SIGMA = 0.2
COMPARE = dict(H.COMPARE)                           # at eps0 = 0.02, no adaptation, sigma sampled from COMPARE_SIGMA
COMPARE_SIGMA = 1.0
COMPARE_CASES = [(N, P, S) for N in (1, 20, 64, 65, 130) for P in (2, 5) for S in (1, 3)]


def case(N, P, S, seed=5):
    """The data, the external measurements and the starting points for P participants x S joint chains of N trials (tools/wiener_hmc_host.py's
    case; extdata = the boundary the data were drawn near, 0.8 .. 1.6, plus noise of the order of sigma) -> (data [P, N, 2], extdata [P],
    theta [P S, 5])."""
    data, theta = H.case(N, C=P * S, D=P, seed=seed + 100 * P + S)
    ext = np.random.default_rng(seed + 7 * N + P).uniform(0.6, 1.8, P)
    return data, ext, theta


def energy_case(N):
    """The energy tests' case: 4 participants x 64 joint chains, sigma held at 0.2."""
    return case(N, 4, 64)


def compare(a, b, theta0):
    """Two runs of the same joint chains -> (the participant chains whose accept decisions agree throughout [C], the largest |log_post
    difference| / (1 + |log_post|) over them, the largest |difference| of their final q, the joint chains all of whose participants and
    sigma steps decided alike [S], the largest |difference| of their final sigma).  q and sigma are compared in the float64 the state
    holds: the float32 draws of so few chains often agree to the last bit, which would set a tolerance of zero."""
    same, dl, _ = H.compare(a, b, theta0)
    S = a["sigma_draws"].shape[0]
    prev = lambda r: np.concatenate([np.full((S, 1), np.float32(COMPARE_SIGMA)), r["sigma_draws"][:, :-1]], 1)
    moved = lambda r: r["sigma_draws"] != prev(r)
    same_k = same.reshape(-1, S).all(0) & np.all(moved(a) == moved(b), axis=1)
    dq = float(np.max(np.abs(a["state"][same, :5] - b["state"][same, :5]))) if same.any() else 0.0
    ds = float(np.max(np.abs(a["sigma"] - b["sigma"])[same_k])) if same_k.any() else 0.0
    return same, dl, dq, same_k, ds


def survey(sanitize=False):
    out = {"tool": "tools/wiener_hmc_joint_host.py", "sanitized": bool(sanitize), "cases": {}, "energy_bar": {}, "device_tolerance": {}}
    with tempfile.TemporaryDirectory() as td:
        if sanitize:                                                    # one small run of every path under ASan + UBSan
            es = build(td, True)
            data, ext, theta = case(65, 5, 3)
            st = H.init_state(theta, data, 3)
            r = run(es, td, data, ext, st, np.full(3, 1.0), n_iter=6, n_adapt=3, n_leapfrog=3, thin=2, seed=1)
            r = run(es, td, data, ext, r["state"], r["sigma"], n_iter=2, n_leapfrog=3, sigma_fixed=True, iter_offset=6)
            assert not r["flagged"].any()
            bad = data.copy()
            bad[1, 0, 1] = 0.0
            assert run(es, td, bad, ext, st, np.full(3, 1.0), n_iter=2, n_leapfrog=3)["flagged"].all()
            out["sanitized_cases"] = 3
        e32, e64 = build(td), build(td, f64=True)
        for N in ENERGY_SHAPES:
            data, ext, theta = energy_case(N)
            r = run(e32, td, data, ext, H.init_state(theta, data, 64, eps0=1e-3), np.full(64, ENERGY_SIGMA), **ENERGY)
            assert not r["flagged"].any() and np.all(np.isfinite(r["state"][:, 11]))
            m = float(np.max(r["state"][:, 11]))
            out["cases"][f"energy_N{N}"] = dict(ENERGY, chains=256, eps=1e-3, sigma=ENERGY_SIGMA, max_abs_energy_error=m,
                                                divergent=int(r["divergent"].sum()))
            out["energy_bar"][str(N)] = H.round_up_1sd(4.0 * m)
        for N, P, S in COMPARE_CASES:
            data, ext, theta = case(N, P, S)
            st = H.init_state(theta, data, S, eps0=0.02)
            sg = np.full(S, COMPARE_SIGMA)
            a, b = run(e32, td, data, ext, st, sg, **COMPARE), run(e64, td, data, ext, st, sg, **COMPARE)
            same, dl, dd, same_k, ds = compare(a, b, theta)
            key = f"N{N}_P{P}_S{S}"
            out["cases"][f"f32_vs_f64_{key}"] = dict(COMPARE, eps=0.02, left_out=int((~same).sum()), left_out_joint=int((~same_k).sum()),
                                                     max_rel_log_post=dl, max_abs_q=dd, max_abs_sigma=ds)
            out["device_tolerance"][key] = dict(log_post_rel=4.0 * dl, q_abs=4.0 * dd, sigma_abs=4.0 * ds)
        cmp_cases = [c for k, c in out["cases"].items() if k.startswith("f32_vs")]
        out["left_out_share"] = sum(c["left_out"] for c in cmp_cases) / float(sum(P * S for _, P, S in COMPARE_CASES))
    return out


if __name__ == "__main__":
    B.cli(survey)
