#!/usr/bin/env python3
"""The chain of csrc/nddm_wiener_hmc.h run on the HOST, without a GPU: the header's own whmc_stage, whmc_log_post, whmc_randoms and
whmc_chain (over nddm_wiener_grad.h's likelihood and nddm_rng.h's Philox and exact Box-Muller) compiled by the host compiler as a
stand-alone program against the stand-in for <hip/hip_runtime.h> of tools/host_build.py, optionally under AddressSanitizer and
UndefinedBehaviorSanitizer.  The 64 lanes are a loop and the butterfly is summed in the kernel's order, so a host chain differs from the
device's only where the hardware's rcp / exp / log differ from the C library's in their last bits.  Two builds: float32 (the kernel's
arithmetic) and `f64=True`, in which the likelihood's headers are compiled with every float a double -- the same expressions and the
same float32-rounded constants, every operation in float64: what bounds the rounding of the float32 operations.

run(exe, td, data [D, N, 2], state [C, 12], ...) -> dict with the C entry point's outputs and the updated state.

Usage: python tools/wiener_hmc_host.py [--sanitize] [--json OUT]      prints one JSON line: the energy error of short trajectories at
eps = 1e-3 (the bar of the energy tests = 4 x the largest), and float32 against float64 over 3 iterations of 4 leapfrog steps (the
tolerance of the device-against-host test = 4 x the largest difference, and the share of chains whose accept decision is within it).
With --censored: the same comparison for NDDM_WIENER_CENSORED's chain on data with 10 % timeouts, per case (censored_survey).
"""
import math
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_build as B  # noqa: E402  (the stand-in header, the compiler call, the command line)

STATE = 12
DC_MIN = 0.05

# what nddm_rng.h names beyond the stand-in (only the exact transform is instantiated; the fast one has to parse)
RNG_SHIM = r"""
#include <hip/hip_runtime.h>
#define __builtin_amdgcn_sqrtf(x) sqrtf(x)
#define __builtin_amdgcn_cosf(x) cosf(6.2831853f * (x))
#define __builtin_amdgcn_sinf(x) sinf(6.2831853f * (x))
#define __builtin_amdgcn_alignbit(a, b, c) 0u
#define WHMC_HOST 1
"""

F64_ON = r"""
#include "nddm_rng.h"
#define WHMC_REAL double
#define float double
#define fabsf fabs
#define fmaxf fmax
#define fminf fmin
#define fmaf fma
#define logf log
#define expf exp
#define exp2f exp2
#define log2f log2
#define sqrtf sqrt
#define __expf exp
#define sinpif(x) sin(M_PI * (x))
#define cospif(x) cos(M_PI * (x))
#include "nddm_wiener_grad.h"
#undef float
#undef fabsf
#undef fmaxf
#undef fminf
#undef fmaf
#undef logf
#undef expf
#undef exp2f
#undef log2f
#undef sqrtf
#undef __expf
#undef sinpif
#undef cospif
"""

MAIN = r"""// usage: wiener_hmc_host in.bin out.bin ; in: 13 int64 (D, N, C, S, n_iter, n_adapt, n_leapfrog, thin, free_mask, seed, chain_offset,
// iter_offset, has_inv_mass), data f32 [D, N, 2], state f64 [C, 12], inv_mass f64 [C, 5] if has_inv_mass; out: draws f32 [C, K, 5],
// log_post f32 [C, K], accept f32 [C], divergent i32 [C], flagged i32 [C], state f64 [C, 12]
#include <cstdio>
#include <cstdlib>
#include <vector>
%s
#include "nddm_wiener_hmc.h"
using namespace nddm;
int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb"); long long h[13]; if (!f || fread(h, 8, 13, f) != 13) return 2;
    const long long D = h[0], N = h[1], C = h[2], S = h[3], n_iter = h[4], n_adapt = h[5], L = h[6], thin = h[7];
    const unsigned mask = (unsigned)h[8]; const unsigned long long seed = (unsigned long long)h[9], coff = h[10], ioff = h[11];
    if (N > WHMC_MAX_TRIALS || N <= 0 || C != D * S || n_iter * L * ((N + 63) / 64) > WHMC_MAX_ROUNDS) return 5;
    const long long K = (long long)((ioff + n_iter) / thin - ioff / thin);
    std::vector<float> data((size_t)D * N * 2), draws((size_t)C * K * 5), lpost((size_t)C * K), acc(C);
    std::vector<double> state((size_t)C * WHMC_STATE), im((size_t)C * 5, 1.0);
    std::vector<int> dv(C), fl(C);
    if (fread(data.data(), 4, data.size(), f) != data.size()) return 3;
    if (fread(state.data(), 8, state.size(), f) != state.size()) return 3;
    if (h[12] && fread(im.data(), 8, im.size(), f) != im.size()) return 3;
    fclose(f);
    std::vector<float2> tile(N);
    for (long long c = 0; c < C; ++c) {
        const WhmcData dat = whmc_stage<HOST_CENSORED>(tile.data(), data.data() + (c / S) * N * 2, (int)N, 0);
        double st[WHMC_STATE], m[5];
        for (int j = 0; j < WHMC_STATE; ++j) st[j] = state[c * WHMC_STATE + j];
        for (int j = 0; j < 5; ++j) m[j] = im[c * 5 + j];
        if (dat.bad || !whmc_state_ok(st, m)) {
            for (long long i = 0; i < K * 5; ++i) draws[c * K * 5 + i] = __builtin_nanf("");
            for (long long i = 0; i < K; ++i) lpost[c * K + i] = __builtin_nanf("");
            acc[c] = __builtin_nanf(""); dv[c] = 0; fl[c] = 1;
            continue;
        }
        const WhmcTally t = whmc_chain<WhmcNoExt, HOST_CENSORED>(st, m, tile.data(), (int)N, dat.T, mask, (unsigned)seed, (unsigned)(seed >> 32), (unsigned)(coff + c), ioff,
                                       (int)n_iter, (int)n_adapt, (int)L, (int)thin, draws.data() + c * K * 5, lpost.data() + c * K, 0, true);
        for (int j = 0; j < WHMC_STATE; ++j) state[c * WHMC_STATE + j] = st[j];
        acc[c] = t.n_sampling ? (float)(t.accept_sum / (double)t.n_sampling) : __builtin_nanf("");
        dv[c] = t.n_divergent; fl[c] = 0;
    }
    f = fopen(argv[2], "wb"); if (!f) return 4;
    fwrite(draws.data(), 4, draws.size(), f); fwrite(lpost.data(), 4, lpost.size(), f); fwrite(acc.data(), 4, acc.size(), f);
    fwrite(dv.data(), 4, dv.size(), f); fwrite(fl.data(), 4, fl.size(), f); fwrite(state.data(), 8, state.size(), f);
    fclose(f);
    return 0;
}
"""


def build(td, sanitize=False, f64=False, censored=False):
    """Compile the stand-alone program into a directory of its own under td -> its path.  censored: NDDM_WIENER_CENSORED's chain."""
    sub = os.path.join(td, ("f64" if f64 else "f32") + ("_censored" if censored else ""))
    os.makedirs(sub)
    switch = "#define HOST_CENSORED %s\n" % ("true" if censored else "false")
    return B.build(sub, MAIN % (switch + RNG_SHIM + (F64_ON if f64 else "")), "wiener_hmc_host", sanitize)


def kept(iter_offset, n_iter, thin):
    return (iter_offset + n_iter) // thin - iter_offset // thin


def run(exe, td, data, state, chains_per_dataset=1, inv_mass=None, n_iter=1, n_adapt=0, n_leapfrog=16, thin=1, free_mask=31, seed=0,
        chain_offset=0, iter_offset=0):
    """The C entry point's call on the host -> {'draws' [C, K, 5], 'log_post' [C, K], 'accept' [C], 'divergent' [C], 'flagged' [C],
    'state' [C, 12]} (numpy; state is a new array)."""
    data = np.ascontiguousarray(data, np.float32)
    state = np.ascontiguousarray(state, np.float64)
    D, N, _ = data.shape
    C = state.shape[0]
    assert state.shape == (C, STATE) and C == D * chains_per_dataset
    K = kept(iter_offset, n_iter, thin)
    return B.exchange(exe, [D, N, C, chains_per_dataset, n_iter, n_adapt, n_leapfrog, thin, free_mask, seed, chain_offset, iter_offset,
                            inv_mass is not None],
                      [data, state] + ([] if inv_mass is None else [np.ascontiguousarray(inv_mass, np.float64).reshape(C, 5)]),
                      (("draws", np.float32, (C, K, 5)), ("log_post", np.float32, (C, K)), ("accept", np.float32, (C,)),
                       ("divergent", np.int32, (C,)), ("flagged", np.int32, (C,)), ("state", np.float64, (C, STATE))))


def init_state(theta, data, chains_per_dataset=1, eps0=0.05, free=31, censored=False):
    """theta [C, 5] in the model's columns -> the state [C, 12] a chain starts from (adaptation at its beginning)."""
    sys.path.insert(0, ROOT)
    from bayesflow_nddms_amd import mcmc
    return mcmc.make_state(theta, np.repeat(np.asarray(data), chains_per_dataset, 0), eps0=eps0, free=free, censored=censored)


def censor(data, share=0.1, seed=0, t_censor=1.2):
    """A copy of `data` [D, N, 2] with about `share` of each data set's trials (one at least) turned into timeouts (choice 0) at
    rt = t_censor + 0.3: the censored tests' data.  Which trials: the data set's slowest responses, as a horizon would take them."""
    d = np.array(data, np.float32)
    k = max(1, int(round(share * d.shape[1])))
    for i in range(d.shape[0]):
        idx = np.argsort(-d[i, :, 0], kind="stable")[:k]
        d[i, idx, 0] = np.float32(t_censor + 0.3)
        d[i, idx, 1] = 0.0
    return d


ENERGY_SHAPES = (1, 20, 64, 65, 130)      # one lane, a partial first round, a full round, a second round of one lane, a third round
PROFILE = os.path.join(ROOT, "profiles", "r17_wiener_hmc_host.json")


def case(N, C=256, D=4, seed=5):
    """The data and the starting points of the energy and device-against-host tests for N trials: C chains on D data sets, started at
    moderate values (drift +-1, boundary .8 .. 1.6, beta .4 .. .6, tau .1 .. .6 of the smallest rt, dc .8 .. 1.25) -> (data [D, N, 2],
    theta [C, 5])."""
    data = example_data(D, N, seed + N)
    rng = np.random.default_rng(seed + 1000 + N)
    S = C // D
    th = np.empty((D, S, 5))
    th[..., 0] = rng.uniform(-1.0, 1.0, (D, S))
    th[..., 1] = rng.uniform(0.8, 1.6, (D, S))
    th[..., 2] = rng.uniform(0.4, 0.6, (D, S))
    th[..., 3] = rng.uniform(0.1, 0.6, (D, S)) * np.minimum(data[..., 0].min(1), 1.5)[:, None]
    th[..., 4] = rng.uniform(0.8, 1.25, (D, S))
    return data, th.reshape(-1, 5)


ENERGY = dict(n_iter=4, n_leapfrog=8, seed=11)       # at eps0 = 1e-3, no adaptation
COMPARE = dict(n_iter=3, n_leapfrog=4, seed=13)      # at eps0 = 0.02, no adaptation: the device-against-host comparison


def moved(draws, theta0):
    """draws [C, K, 5] from theta0 [C, 5] at thin 1 -> bool [C, K]: the iteration's proposal was accepted (the draw differs from the one
    before).  Two runs of one chain whose patterns differ took different accept decisions somewhere."""
    prev = np.concatenate([np.asarray(theta0, np.float32)[:, None, :], draws[:, :-1, :]], 1)
    return np.any(draws != prev, axis=2)


def compare(a, b, theta0):
    """Two runs of the same chains (dicts of run) -> (the chains whose accept decisions agree throughout [C], the largest |log_post
    difference| / (1 + |log_post|) and the largest |draw difference| over those chains)."""
    same = np.all(moved(a["draws"], theta0) == moved(b["draws"], theta0), axis=1)
    la, lb = a["log_post"].astype(np.float64)[same], b["log_post"].astype(np.float64)[same]
    dl = float(np.max(np.abs(la - lb) / (1.0 + np.abs(lb)))) if same.any() else 0.0
    dd = float(np.max(np.abs(a["draws"].astype(np.float64) - b["draws"])[same])) if same.any() else 0.0
    return same, dl, dd


def example_data(D, N, seed):
    """D data sets of N (rt, choice) trials, choice +-1, from moderate basic_ddm_dc parameters: a plain Euler-Maruyama walk in numpy
    (dt 1 ms), which is all a sampler's test data need to be."""
    rng = np.random.default_rng(seed)
    out = np.zeros((D, N, 2), np.float32)
    for d in range(D):
        v, a, b, tau = rng.uniform(-1.5, 1.5), rng.uniform(0.8, 1.6), rng.uniform(0.4, 0.6), rng.uniform(0.2, 0.4)
        x = np.full(N, b * a)
        t = np.zeros(N)
        ch = np.zeros(N)
        live = np.ones(N, bool)
        dt = 1e-3
        while live.any():
            x[live] += v * dt + math.sqrt(dt) * rng.standard_normal(int(live.sum()))
            t[live] += dt
            up, lo = live & (x >= a), live & (x <= 0)
            ch[up], ch[lo] = 1.0, -1.0
            live &= ~(up | lo)
        out[d, :, 0] = t + tau
        out[d, :, 1] = ch
    return out


def round_up_1sd(x):
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-12) * 10.0 ** e


def survey(sanitize=False):
    out = {"tool": "tools/wiener_hmc_host.py", "sanitized": bool(sanitize), "cases": {}, "energy_bar": {}}
    with tempfile.TemporaryDirectory() as td:
        e32, e64 = build(td, sanitize), build(td, sanitize, f64=True)
        for N in ENERGY_SHAPES:
            data, theta = case(N)
            r = run(e32, td, data, init_state(theta, data, 64, eps0=1e-3), 64, **ENERGY)
            assert not r["flagged"].any() and np.all(np.isfinite(r["state"][:, 11]))
            m = float(np.max(r["state"][:, 11]))
            out["cases"][f"energy_N{N}"] = dict(ENERGY, chains=256, eps=1e-3, max_abs_energy_error=m, divergent=int(r["divergent"].sum()))
            out["energy_bar"][str(N)] = round_up_1sd(4.0 * m)          # 4 x: the hardware transcendentals' last ulp
        tol_lp = tol_dr = 0.0
        for N in ENERGY_SHAPES:
            data, theta = case(N)
            st = init_state(theta, data, 64, eps0=0.02)
            a, b = run(e32, td, data, st, 64, **COMPARE), run(e64, td, data, st, 64, **COMPARE)
            same, dl, dd = compare(a, b, theta)
            out["cases"][f"f32_vs_f64_N{N}"] = dict(COMPARE, chains=256, eps=0.02, left_out=int((~same).sum()), max_rel_log_post=dl, max_abs_draw=dd)
            tol_lp, tol_dr = max(tol_lp, dl), max(tol_dr, dd)
        out["device_tolerance_log_post_rel"] = round_up_1sd(4.0 * tol_lp)
        out["device_tolerance_draw_abs"] = round_up_1sd(4.0 * tol_dr)
    return out


CENSORED_PROFILE = os.path.join(ROOT, "profiles", "r22_wiener_censored_hmc_host.json")


def censored_case(N, C=256, D=4):
    """case(N) with about 10 % of every data set's trials timeouts (censor) -> (data [D, N, 2], theta [C, 5])."""
    data, theta = case(N, C=C, D=D)
    return censor(data), theta


def compare_q(a, b, theta0):
    """compare() with the final q (the float64 the state holds) in the draws' place: the float32 draws of two close runs often agree to
    the last bit, which would set a tolerance of zero."""
    same, dl, _ = compare(a, b, theta0)
    dq = float(np.max(np.abs(a["state"][same, :5] - b["state"][same, :5]))) if same.any() else 0.0
    return same, dl, dq


def censored_survey(sanitize=False):
    """NDDM_WIENER_CENSORED's chain: float32 against float64 over 3 iterations of 4 leapfrog steps for every case of the device-against-host
    test (its tolerance = 4 x that case's difference, on log_post and on the final q), and the energy error at eps = 1e-3.  --sanitize runs
    one small case through a build under AddressSanitizer and UndefinedBehaviorSanitizer first (a stand-alone program)."""
    out = {"tool": "tools/wiener_hmc_host.py --censored", "sanitized": bool(sanitize), "cases": {}, "device_tolerance": {}}
    with tempfile.TemporaryDirectory() as td:
        if sanitize:
            data, theta = censored_case(65, C=8, D=4)
            r = run(build(os.path.join(td, "san"), True, censored=True), td, data, init_state(theta, data, 2, censored=True), 2, n_iter=6, n_adapt=3,
                    n_leapfrog=4, seed=3)
            assert not r["flagged"].any() and np.all(np.isfinite(r["draws"]))
        e32, e64 = build(td, censored=True), build(td, f64=True, censored=True)
        for N in ENERGY_SHAPES:
            data, theta = censored_case(N)
            r = run(e32, td, data, init_state(theta, data, 64, eps0=1e-3, censored=True), 64, **ENERGY)
            assert not r["flagged"].any()
            st = init_state(theta, data, 64, eps0=0.02, censored=True)
            a, b = run(e32, td, data, st, 64, **COMPARE), run(e64, td, data, st, 64, **COMPARE)
            same, dl, dq = compare_q(a, b, theta)
            out["cases"][f"N{N}"] = dict(COMPARE, chains=256, eps=0.02, timeouts_per_set=int((data[0, :, 1] == 0).sum()), left_out=int((~same).sum()),
                                         max_rel_log_post=dl, max_abs_q=dq, max_abs_energy_error_at_eps_1em3=float(np.max(r["state"][:, 11])))
            out["device_tolerance"][f"N{N}"] = {"log_post_rel": 4.0 * dl, "q_abs": 4.0 * dq}
    return out


if __name__ == "__main__":
    if "--censored" in sys.argv:
        sys.argv.remove("--censored")
        B.cli(censored_survey)
    else:
        B.cli(survey)
