#!/usr/bin/env python3
"""Rate of the joint sampler (nddm_wiener_hmc_joint; csrc/nddm_wiener_hmc_joint.h) at the shape of the reference's alpha_not_scaled fit --
100 participants x 6 joint chains x 100 trials, 16 leapfrog steps (alpha_not_scaled.py:138-259) -- beside the independent sampler
(nddm_wiener_hmc) at the same shape, in the same run.  Three routes, alternating, after a warm-up of each; every figure is the MEDIAN of
three timed runs (a host clock around work that ends in a device synchronise):

    independent   nddm_wiener_hmc: all the iterations in ONE launch
    joint         nddm_wiener_hmc_joint: a participant launch and a sigma launch per iteration
    joint_fixed   nddm_wiener_hmc_joint with NDDM_HMC_SIGMA_FIXED: the participant launch alone

joint_fixed - independent is what one launch per iteration costs (the gap, the data set staged again, the log posterior evaluated at the
incoming point: 17 gradients against 16); joint - joint_fixed is the sigma kernel with its gap.  The bar: joint <= 2 x independent.

Usage: python tools/wiener_hmc_joint_rate.py [--json OUT] [--iters 4096]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

P, CHAINS, N, LEAPFROG = 100, 6, 100, 16
EPS = 0.05


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--iters", type=int, default=4096)
    a = ap.parse_args()
    import torch
    import wiener_hmc_host as H
    from bayesflow_nddms_amd import engine, mcmc
    engine.require_device()
    data_np = H.example_data(P, N, 41)
    theta, sigma0 = mcmc.hmc_init_joint(data_np, CHAINS, 1)
    ext_np = np.random.default_rng(2).normal(1.1, 0.4, P)
    per = np.repeat(data_np, CHAINS, 0)
    dev = torch.device("cuda")
    data, ext = torch.as_tensor(data_np).to(dev), torch.as_tensor(ext_np).to(dev)
    kw = dict(n_leapfrog=LEAPFROG, seed=3)
    M = engine.BASIC_DDM_DC
    # every route starts from chains that have found the joint posterior: 300 adapting joint iterations (not timed)
    st = torch.as_tensor(mcmc.make_state(theta.reshape(-1, 5), per, eps0=EPS)).to(dev)
    sg = torch.as_tensor(sigma0).to(dev)
    engine.wiener_hmc_joint(M, data, ext, st, sg, n_iter=300, n_adapt=300, want_draws=False, want_log_post=False, **kw)
    torch.cuda.synchronize()

    def independent():
        r = engine.wiener_hmc(M, data, st.clone(), chains_per_dataset=CHAINS, n_iter=a.iters, n_adapt=0, iter_offset=300, thin=10, **kw)
        return r["accept"].mean()

    def joint(fixed=False):
        r = engine.wiener_hmc_joint(M, data, ext, st.clone(), sg.clone(), n_iter=a.iters, n_adapt=0, iter_offset=300, thin=10, sigma_fixed=fixed, **kw)
        return r["accept"].mean()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc = float(fn())                                               # (reading the value back is the synchronise)
        return time.perf_counter() - t0, acc
    routes = {"independent": independent, "joint": joint, "joint_fixed": lambda: joint(True)}
    for fn in routes.values():
        timed(fn)                                                       # warm-up of each
    runs = {k: [] for k in routes}
    accs = {k: [] for k in routes}
    for _ in range(3):                                                  # alternating
        for k, fn in routes.items():
            t, x = timed(fn)
            runs[k].append(t / a.iters)
            accs[k].append(x)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    out = {"tool": "tools/wiener_hmc_joint_rate.py", "device": torch.cuda.get_device_name(0), "participants": P, "joint_chains": CHAINS, "n_trials": N,
           "n_leapfrog": LEAPFROG, "timed_iterations": a.iters, "runs": 3,
           "seconds_per_iteration_runs": runs, "seconds_per_iteration": med, "mean_accept": {k: float(np.mean(v)) for k, v in accs.items()},
           "joint_over_independent": med["joint"] / med["independent"], "bar": 2.0, "bar_met": med["joint"] <= 2.0 * med["independent"],
           "split_seconds_per_iteration": {"independent_sampler": med["independent"],
                                           "participant_launch_over_independent": med["joint_fixed"] - med["independent"],
                                           "sigma_launch": med["joint"] - med["joint_fixed"]},
           "projected_fit_2000_plus_10000_seconds": {k: 12_000 * v for k, v in med.items()}}
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
